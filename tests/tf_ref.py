"""numpy restatement of docs/temporal_filter.md: the integer pyramid, the block motion search, the weights and the blend of the
motion-compensated temporal pre-filter.  Written from the document, not from csrc/dcvc_tf.hip; the two agree bit for bit
(tests/test_gpu_tf.py).  Frames are [3, Hp, Wp] arrays (float16 / float32) with the H x W picture at the top left."""
import numpy as np

BLOCK = 8
BASE = {1: 102, 2: 77}                    # the base weight in 1/256 units by |distance|
SEARCH = (2, 2, 4)                        # the offsets' range at levels 0, 1, 2


def quant(v):
    """Q0 of samples: clamp(rint(v * 1023), 0, 1023), one fp32 multiply, ties to even, NaN -> 0"""
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.rint(np.asarray(v).astype(np.float32) * np.float32(1023.0))
    r = np.where(np.isnan(r), np.float32(0.0), r)
    return np.clip(r, 0.0, 1023.0).astype(np.int32)


def half(q):
    """the next pyramid level: (a + b + c + d + 2) >> 2 over 2 x 2, source coordinates clamped"""
    h, w = q.shape
    ys = np.minimum(np.arange(2 * ((h + 1) // 2)), h - 1)
    xs = np.minimum(np.arange(2 * ((w + 1) // 2)), w - 1)
    p = q[np.ix_(ys, xs)].astype(np.int32)
    return (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + 2) >> 2


def pyramid(frame, size):
    """[Q0, Q1, Q2] (int32 arrays) of the luma plane of a frame"""
    h, w = size
    q0 = quant(frame[0, :h, :w])
    q1 = half(q0)
    return [q0, q1, half(q1)]


def pyramid_flat(frame, size):
    """Q0 | Q1 | Q2 as one uint16 vector: the layout of dcvc_tf_pyramid"""
    return np.concatenate([q.ravel() for q in pyramid(frame, size)]).astype(np.uint16)


def grid(h, w):
    return (h + BLOCK - 1) // BLOCK, (w + BLOCK - 1) // BLOCK


def key(sad, dy, dx):
    """the total order of the candidates as one integer: (SAD, |dy| + |dx|, dy, dx), lexicographic"""
    return (((np.asarray(sad, np.int64) * 16 + np.abs(dy) + np.abs(dx)) * 16 + (dy + 8)) * 16) + (dx + 8)


def parent_centre(mv_parent, gh, gw):
    """the centres [gh, gw, 2] of a level's blocks: twice the vector of block (by >> 1, bx >> 1) of the coarser level, the
    index clamped to that level's grid"""
    ph, pw = mv_parent.shape[:2]
    by = np.minimum(np.arange(gh) >> 1, ph - 1)
    bx = np.minimum(np.arange(gw) >> 1, pw - 1)
    return 2 * mv_parent[np.ix_(by, bx)]


def search_level(qc, qr, centre, rng):
    """one level: qc, qr [Hl, Wl]; centre [gh, gw, 2] -> (mv [gh, gw, 2] int32, sad [gh, gw] int64)"""
    hl, wl = qc.shape
    gh, gw = grid(hl, wl)
    yc = np.minimum(np.arange(gh * BLOCK), hl - 1).reshape(gh, 1, BLOCK, 1)
    xc = np.minimum(np.arange(gw * BLOCK), wl - 1).reshape(1, gw, 1, BLOCK)
    cur = qc[yc, xc].astype(np.int64)                               # [gh, gw, 8, 8]
    cy, cx = centre[..., 0][:, :, None, None], centre[..., 1][:, :, None, None]
    best = np.full((gh, gw), np.iinfo(np.int64).max, np.int64)
    best_mv = np.zeros((gh, gw, 2), np.int32)
    best_sad = np.zeros((gh, gw), np.int64)
    for dy in range(-rng, rng + 1):
        for dx in range(-rng, rng + 1):
            ry = np.clip(yc + cy + dy, 0, hl - 1)
            rx = np.clip(xc + cx + dx, 0, wl - 1)
            sad = np.abs(cur - qr[ry, rx]).sum(axis=(2, 3))
            k = key(sad, dy, dx)
            better = k < best
            best = np.where(better, k, best)
            best_sad = np.where(better, sad, best_sad)
            best_mv[better] = (centre + np.array([dy, dx]))[better]
    return best_mv, best_sad


def motion(pyr_c, pyr_r):
    """the level-0 vectors and errors of one reference: (mv int16 [gh, gw, 2] as (y, x), err uint32 [gh, gw])"""
    mv = None
    for level in (2, 1, 0):
        gh, gw = grid(*pyr_c[level].shape)
        centre = np.zeros((gh, gw, 2), np.int32) if mv is None else parent_centre(mv, gh, gw)
        mv, sad = search_level(pyr_c[level], pyr_r[level], centre, SEARCH[level])
    return mv.astype(np.int16), sad.astype(np.uint32)


def block_weight(err, dist, level):
    """wb per block, int64"""
    a = np.int64(1) << (8 + level)
    e = np.asarray(err).astype(np.int64)
    wb = (np.int64(BASE[abs(int(dist))]) * (a * a - e * e)) >> (16 + 2 * level)
    return np.where(e < a, wb, 0)


def sample_weight(wb, d, level):
    p = np.int64(1) << (3 + level)
    d = d.astype(np.int64)
    return np.where(d < p, (wb * (p * p - d * d)) >> (6 + 2 * level), 0)


def rcp(n):
    """the fp32 value nearest to 1 / n"""
    return np.float32(1.0) / np.asarray(n).astype(np.float32)          # (IEEE fp32 division: correctly rounded; n <= 614 is exact)


def blend(cur, size, level, weighed):
    """the accumulation: cur against `weighed`, per reference in accumulation order (distance, err [gh, gw] of its blocks,
    r [3, H, W] float32: its samples at the blocks' vectors) -> (out [3, Hp, Wp] in cur's dtype, weight sum (int), Wsum of the
    luma plane [H, W])"""
    h, w = size
    by, bx = np.arange(h)[:, None] >> 3, np.arange(w)[None, :] >> 3
    c = cur[:, :h, :w].astype(np.float32)
    qc = quant(c)
    acc = np.float32(256.0) * c
    wsum = np.full((3, h, w), 256, np.int64)
    for dist, err, r in weighed:
        wgt = sample_weight(block_weight(err, dist, level)[by, bx][None], np.abs(qc - quant(r)), level)
        with np.errstate(invalid="ignore", over="ignore"):
            acc = acc + wgt.astype(np.float32) * r
        wsum = wsum + wgt
    with np.errstate(invalid="ignore", over="ignore"):
        res = (acc * rcp(wsum)).astype(cur.dtype)
    pic = np.where(wsum == 256, cur[:, :h, :w], res)                 # no weight: the bits of c
    hp, wp = cur.shape[1:]
    out = pic[:, np.minimum(np.arange(hp), h - 1)][:, :, np.minimum(np.arange(wp), w - 1)]
    return np.ascontiguousarray(out), int((wsum[0] - 256).sum()), wsum[0]


def filter_frame(cur, refs, dists, size, level, motions=None):
    """-> blend()'s three.  refs / dists in accumulation order.  motions: None or the (mv, err) of every reference, where
    they are known already."""
    h, w = size
    ys, xs = np.arange(h)[:, None], np.arange(w)[None, :]
    by, bx = ys >> 3, xs >> 3
    pyr_c = pyramid(cur, size) if motions is None else None
    weighed = []
    for i, (ref, dist) in enumerate(zip(refs, dists)):
        mv, err = motions[i] if motions is not None else motion(pyr_c, pyramid(ref, size))
        ry = np.clip(ys + mv[by, bx, 0], 0, h - 1)
        rx = np.clip(xs + mv[by, bx, 1], 0, w - 1)
        weighed.append((dist, err, ref[:, ry, rx].astype(np.float32)))
    return blend(cur, size, level, weighed)


def window(n_frames, radius):
    """per frame t the (index, distance) list in accumulation order -1, +1, -2, +2 (what prefilter.window restates)"""
    return [[(t + d, d) for d in (-1, 1, -2, 2)[:2 * radius] if 0 <= t + d < n_frames] for t in range(n_frames)]


def texture():
    """the test texture of the issue: per plane low-passed standard-normal noise, 3 x 256 x 320 in [0, 1] (float64)"""
    n = np.random.default_rng(7).standard_normal((3, 256, 320))
    fy, fx = np.fft.fftfreq(256)[:, None], np.fft.fftfreq(320)[None, :]
    g = np.exp(-(fy * fy + fx * fx) / (2 * 0.06 ** 2))
    t = np.real(np.fft.ifft2(np.fft.fft2(n, axes=(1, 2)) * g, axes=(1, 2)))
    lo, hi = t.min(axis=(1, 2), keepdims=True), t.max(axis=(1, 2), keepdims=True)
    return (t - lo) / (hi - lo)


def shift(tex, dy, dx, h=136, w=200):
    """the h x w crop at row 60 + dy, column 60 + dx: its content is found at vector (-dy, -dx) from shift (0, 0)"""
    return tex[:, 60 + dy:60 + dy + h, 60 + dx:60 + dx + w]
