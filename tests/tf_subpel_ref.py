"""numpy restatement of the section "Quarter-pel motion" of docs/temporal_filter.md: the taps, the integer interpolation of
the search, the two refinement stages with their penalised rank, the fp32 interpolation of the blend, and the filter and the
level's choice with the refined vectors.  Written from the document, not from csrc/dcvc_tf_subpel.hip; the two agree bit for
bit (tests/test_gpu_tf_subpel.py).  The pyramid, the whole-pel search, the weights and the level rule are tf_ref's and
tf_auto_ref's."""
import numpy as np

import tf_auto_ref as A
import tf_ref as R

TAPS = np.array([[0, 0, 0, 64, 0, 0, 0, 0],
                 [-1, 4, -10, 58, 17, -5, 1, 0],
                 [-1, 4, -11, 40, 40, -11, 4, -1],
                 [0, 1, -5, 17, 58, -10, 4, -1]], np.int32)
SIXTY_FOURTH = np.float32(0.015625)


def split(m):
    """a quarter-pel component -> (whole part: the floor, phase 0 .. 3)"""
    m = np.asarray(m).astype(np.int32)
    return m >> 2, m & 3


# ---------------------------------------------------------------------------------- the search's integer interpolation
def interp_int(q0r, yc, xc, my, mx):
    """the integer sample of Q0 plane q0r at positions (yc, xc) - clamped to the picture already - and quarter-pel vectors
    (my, mx); all four broadcast against each other -> int32 codes 0 .. 1023"""
    h, w = q0r.shape
    iy, fy = split(my)
    ix, fx = split(mx)
    q = q0r.astype(np.int32)
    v = 0
    for j in range(8):
        rows = np.clip(yc + iy + j - 3, 0, h - 1)
        hj = 0
        for k in range(8):
            hj = hj + TAPS[fx, k] * q[rows, np.clip(xc + ix + k - 3, 0, w - 1)]
        v = v + TAPS[fy, j] * hj
    return np.clip((v + 2048) >> 12, 0, 1023).astype(np.int32)


def sad_q(qc, qr, mvq):
    """SAD per block of the level-0 grid at the quarter-pel vectors mvq [gh, gw, 2] -> int64 [gh, gw]"""
    h, w = qc.shape
    gh, gw = R.grid(h, w)
    yc = np.minimum(np.arange(gh * R.BLOCK), h - 1).reshape(gh, 1, R.BLOCK, 1)
    xc = np.minimum(np.arange(gw * R.BLOCK), w - 1).reshape(1, gw, 1, R.BLOCK)
    my, mx = mvq[..., 0][:, :, None, None].astype(np.int32), mvq[..., 1][:, :, None, None].astype(np.int32)
    return np.abs(qc[yc, xc].astype(np.int64) - interp_int(qr, yc, xc, my, mx)).sum(axis=(2, 3))


def rank(sad, dy, dx):
    """R of a candidate: its SAD, plus an eighth of it where the candidate is not the stage's centre"""
    sad = np.asarray(sad).astype(np.int64)
    return sad if dy == 0 and dx == 0 else sad + (sad >> 3)


def stage(qc, qr, centre, step):
    """one stage: the nine candidates centre + (dy, dx), dy and dx in {-step, 0, step}; the winner is the lexicographic
    minimum of (R, |dy| + |dx|, dy, dx) -> (vectors [gh, gw, 2] int32, the winners' own SADs int64)"""
    best = best_mv = best_sad = None
    for dy in (-step, 0, step):
        for dx in (-step, 0, step):
            cand = centre + np.array([dy, dx], np.int32)
            sad = sad_q(qc, qr, cand)
            k = R.key(rank(sad, dy, dx), dy, dx)
            if best is None:
                best, best_mv, best_sad = k, cand.copy(), sad
                continue
            better = k < best
            best = np.where(better, k, best)
            best_sad = np.where(better, sad, best_sad)
            best_mv[better] = cand[better]
    return best_mv, best_sad


def refine(qc, qr, mv, subpel):
    """the refinement of one reference's level-0 vectors mv [gh, gw, 2]: stage H (step 2) around 4 * mv, with subpel 2 stage
    Q (step 1) around its winner -> (mvq int16 [gh, gw, 2] in quarter pels, errq uint32 [gh, gw])"""
    if subpel not in (1, 2):
        raise ValueError(f"subpel {subpel!r}: 1 or 2")
    mvq, errq = stage(qc, qr, 4 * mv.astype(np.int32), 2)
    if subpel == 2:
        mvq, errq = stage(qc, qr, mvq, 1)
    return mvq.astype(np.int16), errq.astype(np.uint32)


def motion(pyr_c, pyr_r, subpel):
    """(mvq, errq) of one reference from the two pyramids: tf_ref's search, then the refinement"""
    mv, _ = R.motion(pyr_c, pyr_r)
    return refine(pyr_c[0], pyr_r[0], mv, subpel)


# ---------------------------------------------------------------------------------- the blend's fp32 interpolation
def _taps_f32(f, v):
    """per element the phase-f filter of the eight values v[0 .. 7] (float32 arrays): the sum in rising tap order over the
    non-zero taps, begun with the first product, every multiply and add its own fp32 operation, times 1 / 64"""
    out = None
    for phase in (1, 2, 3):
        acc = None
        for k in range(8):
            if TAPS[phase, k] == 0:
                continue
            p = np.float32(TAPS[phase, k]) * v[k]
            acc = p if acc is None else acc + p
        acc = acc * SIXTY_FOURTH
        out = acc if out is None else np.where(f == phase, acc, out)
    return np.where(f == 0, v[3], out)


def interp_f32(ref, size, mvq):
    """the interpolated reference samples r [3, H, W] (float32) of the frame ref at the blocks' quarter-pel vectors
    mvq [gh, gw, 2]; phase (0, 0) has the bits of the sample"""
    h, w = size
    ys, xs = np.arange(h)[:, None], np.arange(w)[None, :]
    by, bx = ys >> 3, xs >> 3
    iy, fy = split(mvq[by, bx, 0])
    ix, fx = split(mvq[by, bx, 1])
    s = ref[:, :h, :w].astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        g = []
        for j in range(8):
            rows = np.clip(ys + iy + j - 3, 0, h - 1)
            g.append(_taps_f32(fx[None], [s[:, rows, np.clip(xs + ix + k - 3, 0, w - 1)] for k in range(8)]))
        return _taps_f32(fy[None], g)


def filter_frame(cur, refs, dists, size, level, subpel=2, motions=None, samples=None):
    """tf_ref.filter_frame with the refined vectors: -> tf_ref.blend()'s three.  motions: None or the (mvq, errq) of every
    reference; samples: None or interp_f32 of every reference at those vectors, where already made"""
    pyr_c = R.pyramid(cur, size) if motions is None else None
    weighed = []
    for i, (ref, dist) in enumerate(zip(refs, dists)):
        mvq, errq = motions[i] if motions is not None else motion(pyr_c, R.pyramid(ref, size), subpel)
        weighed.append((dist, errq, samples[i] if samples is not None else interp_f32(ref, size, mvq)))
    return R.blend(cur, size, level, weighed)


# ---------------------------------------------------------------------------------- the level from the picture
def estimate(cur, refs, dists, size, subpel=2):
    """tf_auto_ref.estimate with errq as the temporal tables -> (the four integers, the (mvq, errq) of every reference)"""
    pyr = R.pyramid(cur, size)
    motions = [motion(pyr, R.pyramid(r, size), subpel) for r in refs]
    return A.noise(pyr[0], [m[1] for m in motions], dists), motions


def filter_auto(cur, refs, dists, size, subpel=2):
    """tf_auto_ref.filter_auto with the refined vectors -> (out, weight sum, the four integers or None)"""
    if not refs:
        out, total, _ = R.filter_frame(cur, [], [], size, 3)
        return out, total, None
    four, motions = estimate(cur, refs, dists, size, subpel)
    if four[0] == 0:
        out, total, _ = R.filter_frame(cur, [], [], size, 3)
    else:
        out, total, _ = filter_frame(cur, refs, dists, size, four[0], subpel, motions)
    return out, total, four


# ---------------------------------------------------------------------------------- material
def fourier_shift(tex, dy, dx):
    """the periodic texture [3, Hy, Wx] displaced by (dy, dx) pels, fractions included: out[y][x] = tex[y - dy][x - dx]"""
    fy, fx = np.fft.fftfreq(tex.shape[1])[:, None], np.fft.fftfreq(tex.shape[2])[None, :]
    ramp = np.exp(-2j * np.pi * (fy * dy + fx * dx))
    return np.real(np.fft.ifft2(np.fft.fft2(tex, axes=(1, 2)) * ramp, axes=(1, 2)))


def moving(tex, t, per_frame, h=136, w=200):
    """frame t of material moving `per_frame` = (dy, dx) pels per frame: the crop of tf_ref.shift at (0, 0) of the texture
    displaced by t * per_frame (an integer displacement is tf_ref.shift(tex, -t * dy, -t * dx))"""
    return R.shift(fourier_shift(tex, t * per_frame[0], t * per_frame[1]), 0, 0, h, w)
