"""numpy restatement of dcvc_resize_frame (csrc/dcvc_resize.hip, docs/reduced_resolution.md) over tables from
opendcvc_amd.resize.filter_taps: fp32 multiply and add in tap order (numpy rounds every float32 product and sum, so no
fused multiply-add), source indices clamped into the valid region, the intermediate kept in fp32, ONE rounding to the
storage type, the output's padding the replicate pad of its valid region."""
import numpy as np

from opendcvc_amd.resize import filter_taps


def _pass(x, first, coef, axis):
    """x float32 [..]; along `axis`: out[j] = c[j][0] * x[i_0], then out = out + c[j][k] * x[i_k], i_k = clip(first[j] + k)"""
    n = x.shape[axis]
    first = np.asarray(first, np.int64)
    coef = np.asarray(coef, np.float32)
    shape = [1] * x.ndim
    shape[axis] = len(first)
    acc = None
    for k in range(coef.shape[1]):
        term = coef[:, k].reshape(shape) * np.take(x, np.clip(first + k, 0, n - 1), axis=axis)
        acc = term if acc is None else acc + term
        assert acc.dtype == np.float32
    return acc


def resize_tables_ref(x, size_in, tables_h, tables_v, padded_out=None):
    """x [3, Hp, Wp] (float16 / float32) with the valid region size_in at its top left; tables_h / tables_v = (first, coef)
    per output column / row -> [3, HOp, WOp] in x's dtype (padded_out = (HOp, WOp), default: no padding)"""
    H, W = size_in
    v = np.asarray(x)[:, :H, :W].astype(np.float32)
    t = _pass(v, tables_h[0], tables_h[1], 2)                  # horizontal, every valid source row
    o = _pass(t, tables_v[0], tables_v[1], 1).astype(x.dtype)
    HO, WO = o.shape[1:]
    HOp, WOp = padded_out or (HO, WO)
    return np.pad(o, ((0, 0), (0, HOp - HO), (0, WOp - WO)), mode="edge")


def resize_ref(x, size_in, size_out, name, pad_to=1):
    """the restatement with filter_taps' tables, the output padded to a multiple of pad_to"""
    (H, W), (HO, WO) = size_in, size_out
    pad = lambda n: n + (-n) % pad_to
    return resize_tables_ref(x, size_in, filter_taps(name, W, WO), filter_taps(name, H, HO), (pad(HO), pad(WO)))
