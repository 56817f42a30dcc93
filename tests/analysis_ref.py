"""numpy restatement of the frame analysis behind the scene-cut decision (csrc/dcvc_analysis.hip, include/dcvc_amd.h
dcvc_frame_analyze): per luma sample ONE float32 multiply by 1023, round to nearest even, clamp to 0 .. 1023 (a NaN
counts as 0), then integers only - 8 x 8 block sums (the low-resolution plane), inter = sum |L - L_prev|, intra = sum of
the smaller of the differences to the left and the top neighbour (first row: left only, first column: top only, block
(0, 0): nothing), total = sum L."""
import numpy as np


def quantise(luma):
    """luma: [H, W] float16 / float32 -> int64 samples 0 .. 1023"""
    v = np.asarray(luma).astype(np.float32)                 # the storage type converted to fp32 (exact)
    with np.errstate(invalid="ignore", over="ignore"):
        p = (v * np.float32(1023.0)).astype(np.float32)     # one fp32 product
        q = np.fmin(np.fmax(np.rint(p), np.float32(0.0)), np.float32(1023.0))     # fmax / fmin drop a NaN
    return q.astype(np.int64)


def lowres(luma):
    """-> [H/8, W/8] int64 block sums (each at most 64 * 1023 = 65472: the kernel stores uint16)"""
    q = quantise(luma)
    h, w = q.shape
    assert h % 8 == 0 and w % 8 == 0 and h >= 8 and w >= 8
    return q.reshape(h // 8, 8, w // 8, 8).sum(axis=(1, 3))


def stats(L, L_prev=None):
    """-> (inter, intra, total, blocks) as Python integers"""
    L = np.asarray(L, np.int64)
    inter = 0 if L_prev is None else int(np.abs(L - np.asarray(L_prev, np.int64)).sum())
    left = np.abs(L[:, 1:] - L[:, :-1])          # block (by, bx + 1) against its left neighbour
    top = np.abs(L[1:, :] - L[:-1, :])           # block (by + 1, bx) against its top neighbour
    intra = int(np.minimum(left[1:, :], top[:, 1:]).sum())     # by > 0 and bx > 0
    intra += int(left[0, :].sum())                             # first row
    intra += int(top[:, 0].sum())                              # first column
    return inter, intra, int(L.sum()), int(L.size)


def analyze(luma, L_prev=None):
    """-> (L, (inter, intra, total, blocks))"""
    L = lowres(luma)
    return L, stats(L, L_prev)


def is_cut(inter, intra, has_prev, scenecut):
    return bool(has_prev and 100 * int(inter) >= int(scenecut) * max(int(intra), 1))


def two_scene_frames(h, w, n=12, cut=5, seeds=(3, 11)):
    """the project's synthetic material with one seed change: (seed 3, idx 0 .. cut-1) then (seed 11, idx cut .. n-1),
    float32 [1, 3, h, w] each"""
    from opendcvc_amd import weights
    return [weights.synthetic_frame_yuv444(h, w, i, seeds[0] if i < cut else seeds[1]) for i in range(n)]
