"""numpy restatement of csrc/dcvc_repeat.hip (docs/frame_repeat.md): the largest sample difference of two model frames per
plane, as the bits of the fp32 difference."""
import numpy as np


def maxdiff(a, b, H, W):
    """a, b: model frames [3][Hp][Wp] of float16 or float32 -> uint32 [4]: per plane the max over the H x W picture of the
    bits of |float32(a) - float32(b)|, then 0.  The keys of non-negative floats order as the floats do; a NaN's key lies
    above +inf's 0x7f800000."""
    with np.errstate(invalid="ignore"):          # (inf - inf, NaN - x: the NaN is the answer)
        d = np.abs(a[:, :H, :W].astype(np.float32) - b[:, :H, :W].astype(np.float32))
    out = np.zeros(4, np.uint32)
    out[:3] = np.ascontiguousarray(d).view(np.uint32).reshape(3, -1).max(axis=1)
    return out


def is_repeat(keys, tol_codes):
    """the detector's rule on maxdiff's words: all three maxima <= float32(tol_codes) / float32(255), in fp32"""
    tol = np.float32(tol_codes) / np.float32(255.0)
    return bool(np.all(np.asarray(keys[:3], np.uint32).view(np.float32) <= tol))
