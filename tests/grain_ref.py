"""numpy restatement of docs/film_grain.md: the white field, the shaped field, the application to a model frame and the
estimator's table.  Written from the doc, shares no code with opendcvc_amd/grain.py or csrc/dcvc_grain.hip."""
import numpy as np

VAR_WHITE = 21845                                   # 4 * (256^2 - 1) / 12
TAPS = ((1,), (1, 2, 1), (1, 4, 6, 4, 1))
GAIN = (3547, 591, 51)
FLAT_T = 1 << 26


def white(seed, t, c, y0, x0, h, w):
    """n(t, c, y, x) for y0 <= y < y0 + h, x0 <= x < x0 + w (y0, x0 >= -2) -> int32 [h, w]"""
    assert y0 >= -2 and x0 >= -2
    M = np.uint64(0xFFFFFFFF)
    a = np.uint64(seed | c << 16 | (t & 0x3FFF) << 18)
    yy = (np.arange(y0, y0 + h, dtype=np.int64) + 2).astype(np.uint64)[:, None]
    xx = (np.arange(x0, x0 + w, dtype=np.int64) + 2).astype(np.uint64)[None, :]
    hh = (a * np.uint64(0x9E3779B1) + yy * np.uint64(0x85EBCA77) + xx * np.uint64(0xC2B2AE3D)) & M
    hh ^= hh >> np.uint64(16)
    hh = (hh * np.uint64(0x7FEB352D)) & M
    hh ^= hh >> np.uint64(15)
    hh = (hh * np.uint64(0x846CA68B)) & M
    hh ^= hh >> np.uint64(16)
    b = lambda k: ((hh >> np.uint64(8 * k)) & np.uint64(255)).astype(np.int32)
    return b(0) + b(1) + b(2) + b(3) - 510


def shaped(seed, corr, t, c, h, w):
    """g(t, c, y, x) over 0 <= y < h, 0 <= x < w -> int64 [h, w]"""
    taps = TAPS[corr]
    r = len(taps) // 2
    n = white(seed, t, c, -r, -r, h + 2 * r, w + 2 * r).astype(np.int64)
    g = np.zeros((h, w), np.int64)
    for i, a in enumerate(taps):
        for j, b in enumerate(taps):
            g += a * b * n[i:i + h, j:j + w]
    return g


def luma_strength(v, scale_y):
    """v: luma samples (any float type) -> int64 strength per sample"""
    s = np.asarray(scale_y, np.int64)
    with np.errstate(invalid="ignore"):
        q = np.rint(np.fmin(np.fmax(v.astype(np.float32), np.float32(0)), np.float32(1)) * np.float32(255)).astype(np.int64)
    k = np.clip((q - 16) >> 5, 0, 6)
    f = (q - 16) & 31
    mid = (s[k] * (32 - f) + s[k + 1] * f + 16) >> 5
    return np.where(q <= 16, s[0], np.where(q >= 240, s[7], mid))


def apply(x, size, seed, corr, scale_y, scale_cb, scale_cr, t):
    """x [3, Hp, Wp] float16 / float32 -> the frame with grain on its size = (H, W) picture, same dtype"""
    H, W = size
    out = np.array(x, copy=True)
    for c in range(3):
        v = x[c, :H, :W]
        s = luma_strength(v, scale_y) if c == 0 else np.int64((scale_cb, scale_cr)[c - 1])
        p = shaped(seed, corr, t, c, H, W) * GAIN[corr] * s
        assert np.abs(p).max(initial=0) < 2 ** 31
        p = p.astype(np.int32)
        with np.errstate(invalid="ignore", over="ignore"):
            y = (v.astype(np.float32) + p.astype(np.float32) * np.float32(2.0 ** -30)).astype(x.dtype)
        out[c, :H, :W] = np.where((p == 0) | np.isnan(v), v, y)
    return out


def stats(noisy, clean, size):
    """noisy, clean [3, Hp, Wp] -> the table int64 [12, 2]"""
    H, W = size
    bh, bw = H // 16, W // 16
    table = np.zeros((12, 2), np.int64)
    if bh == 0 or bw == 0:
        return table
    blocks = lambda a: a[:bh * 16, :bw * 16].reshape(bh, 16, bw, 16).transpose(0, 2, 1, 3)       # [bh, bw, 16, 16]
    with np.errstate(invalid="ignore"):
        cl = clean[:, :H, :W].astype(np.float32)
        d = noisy[:, :H, :W].astype(np.float32) - cl
        cq = np.fmin(np.fmax(np.rint(cl[0] * np.float32(4096)), np.float32(0)), np.float32(4096)).astype(np.int64)
        dq = np.fmin(np.fmax(np.rint(d * np.float32(4096)), np.float32(-2047)), np.float32(2047)).astype(np.int64)
    cb = blocks(cq)
    sc = cb.sum((2, 3))
    flat = 256 * (cb * cb).sum((2, 3)) - sc * sc <= FLAT_T
    band = np.minimum(sc >> 17, 7)
    V = []
    for c in range(3):
        db = blocks(dq[c])
        sd = db.sum((2, 3))
        V.append(256 * (db * db).sum((2, 3)) - sd * sd)
    db = blocks(dq[0])
    sd = db.sum((2, 3))
    Ch = 65536 * (db[..., :, :-1] * db[..., :, 1:]).sum((2, 3)) - 240 * sd * sd
    Cv = 65536 * (db[..., :-1, :] * db[..., 1:, :]).sum((2, 3)) - 240 * sd * sd
    for k in range(8):
        sel = flat & (band == k)
        table[k] = sel.sum(), V[0][sel].sum()
    for line, q in ((8, V[1]), (9, V[2]), (10, Ch), (11, Cv)):
        table[line] = flat.sum(), q[flat].sum()
    return table


def estimator_picture(dtype=np.float32):
    """the estimator's picture, 144 x 256: 128 rows of eight luma steps of 32 columns at the band centres (16 whole flat
    blocks per band), below them a 16-row full-contrast checker strip; Cb and Cr constant"""
    x = np.empty((3, 144, 256), np.float32)
    x[0, :128] = np.repeat((np.arange(8, dtype=np.float32) + 0.5) / 8, 32)[None, :]
    yy, xx = np.mgrid[128:144, 0:256]
    x[0, 128:] = ((yy + xx) & 1).astype(np.float32)
    x[1], x[2] = 0.5, 0.375
    return x.astype(dtype)
