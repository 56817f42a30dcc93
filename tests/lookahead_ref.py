"""numpy restatement of the frame lookahead (docs/lookahead.md): the pair cost of two low-resolution planes (include/dcvc_amd.h
dcvc_lookahead_cost) - moments, weight and offset, the motion-compensated and the weighted cost - and the cut / flash / fade
policy of opendcvc_amd.lookahead, written from the document with Python integers throughout; plus the synthetic materials
the tests and the document's table use.  The planes are analysis_ref.lowres()'s."""
import numpy as np

import analysis_ref as A

RANGE = 3                   # candidates (dy, dx) in [-RANGE, RANGE]^2
TILE = 8


# ---------------------------------------------------------------------------------- the pair cost
def moments(L):
    """-> (mean, ac) of a plane"""
    L = np.asarray(L, np.int64)
    n = int(L.size)
    mean = (int(L.sum()) + n // 2) // n
    return mean, int(np.abs(L - mean).sum())


def weight_offset(mean_cur, ac_cur, mean_ref, ac_ref):
    w = 64 if ac_ref == 0 else min(max((64 * ac_cur + ac_ref // 2) // ac_ref, 0), 255)
    return w, mean_cur - ((mean_ref * w + 32) >> 6)


def weighted(ref, w, o):
    """wp(r) of every sample; nothing leaves 32 bits before the clamp"""
    ref = np.asarray(ref, np.int64)
    v = ((ref * w + 32) >> 6) + o
    assert int(np.abs(v).max(initial=0)) < 2 ** 31 and int((ref * w + 32).max(initial=0)) < 2 ** 31
    return np.clip(v, 0, 65535)


def _search(cur, ref):
    """sum over the 8 x 8 tiles (partial at the right and bottom edge) of the smallest SAD over the 49 candidates"""
    bh, bw = cur.shape
    ys, xs = np.arange(bh), np.arange(bw)
    th, tw = -(-bh // TILE), -(-bw // TILE)
    sads = []
    for dy in range(-RANGE, RANGE + 1):
        for dx in range(-RANGE, RANGE + 1):
            moved = ref[np.clip(ys + dy, 0, bh - 1)][:, np.clip(xs + dx, 0, bw - 1)]
            d = np.zeros((th * TILE, tw * TILE), np.int64)          # samples that do not exist add nothing
            d[:bh, :bw] = np.abs(cur - moved)
            sads.append(d.reshape(th, TILE, tw, TILE).sum(axis=(1, 3)))
    return int(np.min(np.stack(sads), axis=0).sum())


def cost(cur, ref):
    """-> the eight words of dcvc_lookahead_cost as Python integers: mc, wp, w, o, mean_cur, ac_cur, mean_ref, ac_ref"""
    cur, ref = np.asarray(cur, np.int64), np.asarray(ref, np.int64)
    assert cur.shape == ref.shape and cur.ndim == 2
    mean_cur, ac_cur = moments(cur)
    mean_ref, ac_ref = moments(ref)
    w, o = weight_offset(mean_cur, ac_cur, mean_ref, ac_ref)
    return _search(cur, ref), _search(cur, weighted(ref, w, o)), w, o, mean_cur, ac_cur, mean_ref, ac_ref


# ---------------------------------------------------------------------------------- the policy
def cutlike(c, intra, scenecut):
    return 100 * int(c) >= int(scenecut) * max(int(intra), 1)


class PlaneCosts:
    """what the policy asks of a sequence, answered from its planes: costs(i, j) -> (mc, wp) of frame i against frame j,
    intra(i); `asked` lists the pairs in the order they were first asked for"""

    def __init__(self, planes):
        self.planes = [np.asarray(p, np.int64) for p in planes]
        self._intra = [A.stats(p)[1] for p in self.planes]
        self._cache, self.asked = {}, []

    def costs(self, i, j):
        if (i, j) not in self._cache:
            self._cache[(i, j)] = cost(self.planes[i], self.planes[j])[:2]
            self.asked.append((i, j))
        return self._cache[(i, j)]

    def intra(self, i):
        return self._intra[i]


def decide(costs, n, depth, scenecut):
    """the decisions of an n-frame sequence, every frame decided with the `depth` frames behind it (fewer at the end) ->
    (cuts, flashes, fades, ratios): lists of frame indices, and per frame the deciding figures 100 * cost / max(intra, 1)
    as a dict (mc; ahead: the list rule 2 went through; wp where rule 3 was reached)"""
    cuts, flashes, fades, ratios = [], [], [], [{}]
    anchor, flash_end = 0, 0
    ratio = lambda c, t: 100.0 * c / max(costs.intra(t), 1)
    for t in range(1, n):
        r = {}
        ratios.append(r)
        if t < flash_end:                        # labelled a flash frame: not a cut, the anchor stays
            continue
        mc, wp = costs.costs(t, anchor)
        r["mc"] = ratio(mc, t)
        if not cutlike(mc, costs.intra(t), scenecut):
            anchor = t
            continue
        r["ahead"] = []
        for k in range(1, depth + 1):
            if t + k >= n:
                break
            back = costs.costs(t + k, anchor)[0]
            r["ahead"].append(ratio(back, t + k))
            if not cutlike(back, costs.intra(t + k), scenecut):
                flashes.append(t)
                flash_end = t + k
                break
        if t < flash_end:
            continue
        r["wp"] = ratio(wp, t)
        if not cutlike(wp, costs.intra(t), scenecut):
            fades.append(t)
        else:
            cuts.append(t)
        anchor = t
    return cuts, flashes, fades, ratios


def deciding(ratios):
    """the figures the decisions hung on, flat: each must stand clear of the threshold"""
    out = []
    for r in ratios:
        out += [r[k] for k in ("mc", "wp") if k in r] + r.get("ahead", [])
    return out


def today(planes, scenecut):
    """the frames today's one-pair decision (analysis.is_cut on inter) calls cuts, and its ratios"""
    cuts, ratios = [], [0.0]
    for t in range(1, len(planes)):
        inter, intra, _, _ = A.stats(planes[t], planes[t - 1])
        ratios.append(100.0 * inter / max(intra, 1))
        if A.is_cut(inter, intra, True, scenecut):
            cuts.append(t)
    return cuts, ratios


# ---------------------------------------------------------------------------------- materials (float32 [1, 3, h, w] frames)
def _frame(h, w, i, seed=3):
    from opendcvc_amd import weights
    return weights.synthetic_frame_yuv444(h, w, i, seed)


def _towards(x, alpha, target):
    """alpha * x + (1 - alpha) * target in float32"""
    return (np.float32(alpha) * x + np.float32(1.0 - alpha) * np.float32(target)).astype(np.float32)


def steady(h, w, n=12, seed=3):
    return [_frame(h, w, i, seed) for i in range(n)]


def real_cut(h, w, n=10, cut=5, seeds=(3, 11)):
    return A.two_scene_frames(h, w, n, cut, seeds)


def fade(h, w, target, lead=3, step=0.15):
    """`lead` frames of the scene, then alpha = 1 - step, 1 - 2 step, .. down to 0 towards black (target 0.0) or white (1.0),
    then two more frames of the flat picture -> (frames, the indices of the fading frames: the first flat one is the last)"""
    alphas = [1.0] * lead
    while alphas[-1] > 0.0:
        alphas.append(max(round(alphas[-1] - step, 6), 0.0))
    fading = list(range(lead, len(alphas)))
    alphas += [0.0, 0.0]
    return [_towards(_frame(h, w, i), a, target) for i, a in enumerate(alphas)], fading


def flash(h, w, n=10, at=4, alphas=(0.5, 0.4), left_half_only=False):
    """frames at, at + 1, .. blended towards white with the scene's share alphas; left_half_only: the right half stays"""
    out = []
    for i in range(n):
        x = _frame(h, w, i)
        if at <= i < at + len(alphas):
            y = _towards(x, alphas[i - at], 1.0)
            if left_half_only:
                y[..., w // 2:] = x[..., w // 2:]
            x = y
        out.append(x)
    return out


def pan(h, w, px, n=6):
    """a still (frame 0 of the scene on a wider canvas) seen through a window that moves px pixels per frame"""
    still = _frame(h, w + px * (n - 1), 0)
    return [np.ascontiguousarray(still[..., i * px:i * px + w]) for i in range(n)]


def dissolve(h, w, n=12, start=4, length=5, seeds=(3, 11)):
    """scene seeds[0] cross-fades into scene seeds[1] over `length` frames"""
    out = []
    for i in range(n):
        a = min(max((i - start + 1) / (length + 1.0), 0.0), 1.0)          # the second scene's share
        out.append((np.float32(1.0 - a) * _frame(h, w, i, seeds[0]) + np.float32(a) * _frame(h, w, i, seeds[1])).astype(np.float32))
    return out


def planes_of(frames, dtype=np.float32):
    return [A.lowres(np.asarray(x)[0, 0].astype(dtype)) for x in frames]
