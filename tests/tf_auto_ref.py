"""numpy restatement of the section "Choosing the level from the picture" of docs/temporal_filter.md: the two block tables,
the figure of a table, N, the level rule, and the filter at the chosen level.  Written from the document, not from
csrc/dcvc_tf.hip; integer throughout, so the two agree exactly (tests/test_gpu_tf_auto.py).  The pyramid, the motion search
and the blend are tf_ref's."""
import numpy as np

import tf_ref as R

CLIP = 4095                               # a block value's ceiling: the histograms have 4096 bins
FLOOR = 40                                # N below this: level 0
STEP = 80                                 # level L takes N up to STEP << L


def laplacian_sums(q0):
    """S per 8 x 8 block of a Q0 plane [H, W]: the sum over the block's 64 positions (a position past the picture's edge is
    the edge position) of |corners - 2 edges + 4 centre| of the 3 x 3 neighbourhood, coordinates clamped -> int64 [gh, gw]"""
    h, w = q0.shape
    gh, gw = R.grid(h, w)
    q = q0.astype(np.int64)
    ys, xs = np.arange(h), np.arange(w)
    up, dn = np.maximum(ys - 1, 0), np.minimum(ys + 1, h - 1)
    lf, rt = np.maximum(xs - 1, 0), np.minimum(xs + 1, w - 1)
    resp = (q[np.ix_(up, lf)] + q[np.ix_(up, rt)] + q[np.ix_(dn, lf)] + q[np.ix_(dn, rt)]
            - 2 * (q[np.ix_(up, xs)] + q[np.ix_(dn, xs)] + q[np.ix_(ys, lf)] + q[np.ix_(ys, rt)]) + 4 * q)
    yc = np.minimum(np.arange(gh * R.BLOCK), h - 1)
    xc = np.minimum(np.arange(gw * R.BLOCK), w - 1)
    return np.abs(resp)[np.ix_(yc, xc)].reshape(gh, R.BLOCK, gw, R.BLOCK).sum(axis=(1, 3))


def spatial_table(q0):
    return np.minimum(laplacian_sums(q0) >> 2, CLIP)


def temporal_table(err):
    return np.minimum(np.asarray(err).astype(np.int64), CLIP)


def figure(table):
    """the lower quartile of a table's positive values, 0 where fewer than an eighth of the values are positive"""
    v = np.asarray(table).astype(np.int64).ravel()
    pos = np.sort(v[v > 0])
    if pos.size * 8 < v.size:
        return 0
    return int(pos[pos.size >> 2])


def level_of(n):
    if n < FLOOR:
        return 0
    for level in (1, 2, 3, 4, 5):
        if n <= STEP << level:
            return level
    return 5


def noise(q0, errs, dists):
    """q0: the current frame's Q0; errs / dists: the level-0 SADs [gh, gw] and the distances of the references passed
    -> (level, N, smallest temporal figure or -1, spatial figure)"""
    temporal = [figure(temporal_table(e)) for e, d in zip(errs, dists) if abs(int(d)) == 1]
    spatial = figure(spatial_table(q0))
    t = min(temporal) if temporal else -1
    n = min(temporal + [spatial])
    return level_of(n), n, t, spatial


def estimate(cur, refs, dists, size):
    """frames -> (the four integers, the (mv, err) of every reference)"""
    pyr = R.pyramid(cur, size)
    motions = [R.motion(pyr, R.pyramid(r, size)) for r in refs]
    return noise(pyr[0], [m[1] for m in motions], dists), motions


def filter_auto(cur, refs, dists, size):
    """-> (out, weight sum, the four integers or None); a frame without references is a copy and is not estimated; level 0
    is filter_frame with no references"""
    if not refs:
        out, total, _ = R.filter_frame(cur, [], [], size, 3)
        return out, total, None
    four, motions = estimate(cur, refs, dists, size)
    if four[0] == 0:
        out, total, _ = R.filter_frame(cur, [], [], size, 3)
    else:
        out, total, _ = R.filter_frame(cur, refs, dists, size, four[0], motions)
    return out, total, four


def totals(fours):
    """the eight totals of a sequence's estimated frames: six level counts, the sum of N, the number of frames"""
    t = [0] * 8
    for four in fours:
        if four is not None:
            t[four[0]] += 1
            t[6] += four[1]
            t[7] += 1
    return t
