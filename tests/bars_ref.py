"""numpy restatement of active-area coding (docs/active_area.md; csrc/dcvc_bars.hip): the ordered key of a sample, the
min / max envelope of a set of frames, the extent rule on an envelope, and the window / paste copies.  Everything the
kernels compute is integer min / max or a handful of fp32 operations, so kernels and restatement agree bit for bit."""
import numpy as np


def key(x):
    """ordered keys (uint32) of samples of any float type: u = bits of (float32)x; u ^ 0x80000000 if the sign bit is clear,
    else ~u"""
    u = np.ascontiguousarray(np.asarray(x).astype(np.float32)).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u ^ np.uint32(0x80000000)).astype(np.uint32)


def value(k):
    """the fp32 sample of a key"""
    k = np.asarray(k, np.uint32)
    return np.where(k & np.uint32(0x80000000), k ^ np.uint32(0x80000000), ~k).astype(np.uint32).view(np.float32)


def empty(H, W):
    """the envelope behind a reset: (rowmin[3][H], colmin[3][W], rowmax[3][H], colmax[3][W])"""
    return (np.full((3, H), 0xFFFFFFFF, np.uint32), np.full((3, W), 0xFFFFFFFF, np.uint32),
            np.zeros((3, H), np.uint32), np.zeros((3, W), np.uint32))


def scan(env, x, H, W):
    """folds the valid H x W region of the frame x [3][Hp][Wp] into the envelope -> the new envelope"""
    k = key(np.asarray(x)[:, :H, :W])
    rmin, cmin, rmax, cmax = env
    return (np.minimum(rmin, k.min(axis=2)), np.minimum(cmin, k.min(axis=1)),
            np.maximum(rmax, k.max(axis=2)), np.maximum(cmax, k.max(axis=1)))


def flat_words(env):
    """the envelope as the workspace holds it: one uint32 array"""
    return np.concatenate([a.reshape(-1) for a in env])


def extent(env, tol):
    """the normative rule -> 8 int32 words {found, top, bottom, left, right, c0, c1, c2 (fp32 bits)}"""
    tol = np.float32(tol)
    rmin, cmin, rmax, cmax = (value(a) for a in env)
    H, W = rmin.shape[1], cmin.shape[1]
    out = np.zeros(8, np.int32)
    with np.errstate(invalid="ignore", over="ignore"):
        c = None
        for lo, hi, i in ((rmin, rmax, 0), (rmin, rmax, H - 1), (cmin, cmax, 0), (cmin, cmax, W - 1)):
            if np.all((hi[:, i] - lo[:, i]).astype(np.float32) <= tol):
                c = lo[:, i].astype(np.float32)
                break
        if c is None:
            return out

        def bars(lo, hi):
            return np.all((hi <= (c + tol).astype(np.float32)[:, None]) & (lo >= (c - tol).astype(np.float32)[:, None]), axis=0)

        def leading(b):
            return int(np.argmin(b)) if not b.all() else len(b)

        rows, cols = bars(rmin, rmax), bars(cmin, cmax)
    out[0] = 1
    out[1:5] = leading(rows), leading(rows[::-1]), leading(cols), leading(cols[::-1])
    out[5:8] = c.view(np.int32)
    return out


def _replicate(valid, Hp, Wp):
    H, W = valid.shape[1:]
    return np.pad(valid, ((0, 0), (0, Hp - H), (0, Wp - W)), mode="edge")


def window(x, top, left, HO, WO, HOp, WOp):
    """x [3][Hp][Wp] -> [3][HOp][WOp]: x[top : top + HO, left : left + WO] and its replicate pad"""
    return _replicate(np.asarray(x)[:, top:top + HO, left:left + WO], HOp, WOp)


def paste(x, H, W, top, left, HO, WO, HOp, WOp, colour):
    """x [3][Hp][Wp] with the H x W window -> [3][HOp][WOp]: the colour (fp32, rounded to x's type) with the window at
    (top, left) of the HO x WO picture, and its replicate pad"""
    x = np.asarray(x)
    full = np.empty((3, HO, WO), x.dtype)
    full[:] = np.asarray(colour, np.float32).astype(x.dtype)[:, None, None]
    full[:, top:top + H, left:left + W] = x[:, :H, :W]
    return _replicate(full, HOp, WOp)
