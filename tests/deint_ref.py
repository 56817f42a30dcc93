"""numpy restatement of the deinterlacer (docs/deinterlace.md; csrc/dcvc_deint.hip): the filter, the two decision rules and
the stateful object, operation for operation - every fp32 multiply, add and compare its own, one rounding to the storage type
at the end, 64-bit integer sums.  The kernels are held against it bit for bit (tests/test_gpu_deint.py)."""
import numpy as np

F = np.float32
BIAS = F(1.0) / F(255.0)           # what the straight-up direction is preferred by
HALF = F(0.5)


def fmax(a, b):
    """a > b ? a : b - the document's max: a select, not IEEE maximum (a NaN or an equal pair gives b)"""
    return np.where(a > b, a, b)


def fmin(a, b):
    return np.where(a < b, a, b)


def row_at(y, off, H):
    """row y + off; an offset that leaves [0, H) takes the opposite sign; if that leaves as well it becomes 0"""
    if 0 <= y + off < H:
        return y + off
    if 0 <= y - off < H:
        return y - off
    return y


def missing_rows(H, parity, L):
    return [y for y in range(H) if (y // L) % 2 != parity]


def check_size(H, chroma_lines):
    if chroma_lines not in (1, 2) or H <= 0 or H % (2 * chroma_lines):
        raise ValueError(f"height {H}: a multiple of {2 * chroma_lines} is needed (chroma_lines {chroma_lines})")


def spatial(c, rows, up, dn, W):
    """the edge-directed predictor of the rows `rows` of the fp32 plane c [H, W] -> pr [len(rows), W]"""
    X = np.arange(W)
    col = lambda j: np.clip(X + j, 0, W - 1)
    C = lambda j: c[up][:, col(j)]
    E = lambda j: c[dn][:, col(j)]
    score = lambda j: (np.abs(C(j - 1) - E(-j - 1)) + np.abs(C(j) - E(-j))) + np.abs(C(j + 1) - E(-j + 1))
    pred = lambda j: (C(j) + E(-j)) * HALF
    s, pr = score(0) - BIAS, pred(0)
    for sg in (-1, 1):
        s1 = score(sg)
        take = s1 < s
        s, pr = np.where(take, s1, s), np.where(take, pred(sg), pr)
        s2 = score(2 * sg)
        take2 = take & (s2 < s)
        s, pr = np.where(take2, s2, s), np.where(take2, pred(2 * sg), pr)
    return pr.astype(F)


def filter_plane(cur, prev, H, W, parity, L):
    """one plane: cur / prev [Hp, Wp] in the storage type (prev None: no previous frame) -> the H x W picture, storage type"""
    out = np.array(cur[:H, :W])
    rows = missing_rows(H, parity, L)
    if not rows:
        return out
    c = cur[:H, :W].astype(F)
    up, dn = [row_at(y, -L, H) for y in rows], [row_at(y, L, H) for y in rows]
    with np.errstate(invalid="ignore", over="ignore"):
        pr = spatial(c, rows, up, dn, W)
        if prev is None:
            res = pr
        else:
            P = prev[:H, :W].astype(F)
            up2, dn2 = [row_at(y, -2 * L, H) for y in rows], [row_at(y, 2 * L, H) for y in rows]
            C0, E0 = c[up], c[dn]
            d = (P[rows] + c[rows]) * HALF
            t0 = np.abs(P[rows] - c[rows]) * HALF
            t1 = (np.abs(P[up] - C0) + np.abs(P[dn] - E0)) * HALF
            diff = fmax(t0, t1)
            b = (P[up2] + c[up2]) * HALF - C0
            f = (P[dn2] + c[dn2]) * HALF - E0
            dc, de = d - C0, d - E0
            mx = fmax(fmax(de, dc), fmin(b, f))
            mn = fmin(fmin(de, dc), fmax(b, f))
            diff = fmax(fmax(diff, mn), -mx)
            res = fmin(fmax(pr, d - diff), d + diff)
        out[rows] = res.astype(F).astype(out.dtype)
    return out


def replicate_pad(pic, Hp, Wp):
    H, W = pic.shape[-2:]
    return np.ascontiguousarray(pic[..., np.minimum(np.arange(Hp), H - 1), :][..., np.minimum(np.arange(Wp), W - 1)])


def deinterlace(cur, prev, H, W, parity, chroma_lines, decision=None):
    """cur / prev [3, Hp, Wp] (prev None: none); decision None: always filter, 0: cur's picture passes, else filter ->
    [3, Hp, Wp]: the picture and its replicate pad"""
    check_size(H, chroma_lines)
    Hp, Wp = cur.shape[-2:]
    if decision is not None and not decision:
        return replicate_pad(np.array(cur[:, :H, :W]), Hp, Wp)
    planes = [filter_plane(cur[p], None if prev is None else prev[p], H, W, parity, 1 if p == 0 else chroma_lines)
              for p in range(3)]
    return replicate_pad(np.stack(planes), Hp, Wp)


def quant(v):
    """clamp(rint(v * 1023), 0, 1023), one fp32 multiply, ties to even, NaN -> 0 (tests/tf_ref.py's quant)"""
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.rint(np.asarray(v).astype(F) * F(1023.0))
    r = np.where(np.isnan(r), F(0.0), r)
    return np.clip(r, 0.0, 1023.0).astype(np.int64)


def comb_sums(cur, prev, H, W, parity):
    """luma of cur / prev [3, Hp, Wp] -> (dc, dp) with a previous frame, (dc, ds) without: python ints"""
    q = quant(cur[0, :H, :W])
    rows = [y for y in range(1, H - 1) if y % 2 == parity]
    if not rows:
        return 0, 0
    r = np.asarray(rows)
    dc = int(np.abs(2 * q[r] - q[r - 1] - q[r + 1]).sum())
    if prev is not None:
        qp = quant(prev[0, :H, :W])
        return dc, int(np.abs(2 * q[r] - qp[r - 1] - qp[r + 1]).sum())
    a, b = [row_at(y, -2, H) for y in rows], [row_at(y, 2, H) for y in rows]
    return dc, int(np.abs(2 * q[r] - q[a] - q[b]).sum())


def comb_decision(cur, prev, H, W, parity):
    """1: the frame is interlaced (it is filtered), 0: progressive (it passes)"""
    dc, other = comb_sums(cur, prev, H, W, parity)
    if prev is not None:
        return 0 if 8 * dc < 7 * other else 1
    return 1 if dc > other else 0


class Deinterlacer:
    """opendcvc_amd.deinterlace.Deinterlacer on numpy frames [3, Hp, Wp]"""

    def __init__(self, mode="on", order="tff", chroma_lines=1):
        assert mode in ("on", "auto") and order in ("tff", "bff")
        self.mode, self.parity, self.chroma_lines = mode, 0 if order == "tff" else 1, chroma_lines
        self.judged = self.interlaced = 0
        self.prev = None

    def reset(self):
        self.prev = None

    def filter(self, x, size):
        H, W = size
        check_size(H, self.chroma_lines)
        prev = self.prev
        if prev is not None and (prev[1] != (H, W) or prev[0].shape != x.shape or prev[0].dtype != x.dtype):
            prev = None
        p = None if prev is None else prev[0]
        decision = None
        if self.mode == "auto":
            decision = comb_decision(x, p, H, W, self.parity)
            self.judged += 1
            self.interlaced += decision
        self.prev = (x, (H, W))
        return deinterlace(x, p, H, W, self.parity, self.chroma_lines, decision)

    def counts(self):
        return self.judged, self.interlaced


# ---------------------------------------------------------------------------------- synthetic clips whose truth is known
def texture(h, w, seed, blur=2):
    """a smooth random texture in [0.1, 0.9], float64 [h, w]: uniform noise under two box blurs of 2 * blur + 1 each way"""
    k = 2 * blur + 1
    t = np.random.default_rng(seed).random((h + 4 * blur, w + 4 * blur))
    for _ in range(2):
        t = sum(t[i:t.shape[0] - k + 1 + i] for i in range(k)) / k
        t = sum(t[:, i:t.shape[1] - k + 1 + i] for i in range(k)) / k
    t = (t - t.min()) / (t.max() - t.min())
    return 0.1 + 0.8 * t


def make_clip(kind, frames, H, W, speed=2, vy=0, sigma=0.0, seed=0, parity=0, chroma_lines=1, blur=2):
    """-> (clip, truth): per frame the 8-bit planes of a source file - [3, H, W] for chroma_lines 1 (4:4:4), else (y, u, v) with
    u, v [H / 2, W / 2] (4:2:0) - of a texture that moves `speed` half-pixels to the left and vy rows up per FIELD (speed
    pixels and 2 vy rows per frame).  kind "progressive": every line of frame t shows field time 2 t; "interlaced": the lines
    of the field that comes first (parity) show 2 t, the others 2 t + 1, and in 4:2:0 the chroma rows alternate between the
    fields; "static": time 0 throughout.  sigma: white noise in 8-bit codes, drawn per frame.  truth: the noise-free
    progressive picture at time 2 t, in the same form"""
    assert kind in ("progressive", "interlaced", "static") and H % (2 * chroma_lines) == 0 and W % 2 == 0
    K = 2 * frames
    tex = [texture(H + vy * K, 2 * W + speed * K, seed * 3 + p, blur) for p in range(3)]
    rng = np.random.default_rng(seed + 1000)

    def scene(p, k):                 # plane p at field time k, full resolution
        k = 0 if kind == "static" else k
        return tex[p][vy * k:vy * k + H, speed * k:speed * k + 2 * W:2]

    def code(v, noisy):
        v = v * 255.0 + (rng.normal(0.0, sigma, v.shape) if noisy and sigma else 0.0)
        return np.clip(np.rint(v), 0, 255).astype(np.uint8)

    def picture(t, woven, noisy):
        planes = []
        for p in range(3):
            L = 1 if p == 0 else chroma_lines
            first, second = scene(p, 2 * t), scene(p, 2 * t + 1 if woven else 2 * t)
            if L == 2:
                first, second = first[::2, ::2], second[::2, ::2]
            out = np.array(first)
            rows = np.arange(out.shape[0]) % 2 != parity
            out[rows] = second[rows]
            planes.append(code(out, noisy))
        return np.stack(planes) if chroma_lines == 1 else tuple(planes)

    clip = [picture(t, kind == "interlaced", True) for t in range(frames)]
    truth = [picture(t, False, False) for t in range(frames)]
    return clip, truth


def to_frame(planes, dtype=np.float32, Hp=None, Wp=None, pad=None):
    """8-bit planes of make_clip -> the model frame [3, Hp, Wp] in `dtype`: code / 255 in fp32, 4:2:0 chroma doubled both ways,
    the picture at the top left; pad None: the replicate pad, else that value"""
    if isinstance(planes, tuple):
        planes = np.stack([planes[0]] + [np.repeat(np.repeat(c, 2, 0), 2, 1) for c in planes[1:]])
    pic = (planes.astype(F) / F(255.0)).astype(dtype)
    H, W = pic.shape[-2:]
    Hp, Wp = Hp or H, Wp or W
    if pad is None:
        return np.ascontiguousarray(replicate_pad(pic, Hp, Wp))
    out = np.full((3, Hp, Wp), pad, dtype)
    out[:, :H, :W] = pic
    return out
