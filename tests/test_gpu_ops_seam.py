"""The operator seam's proxies (opendcvc_amd.ops.DepthConvProxy / SubpelConv2xProxy) as the reference's layers call them:
NCHW in and out, fp32 and fp16, forward / forward_with_quant_step / forward_with_cat, at widths that need channel padding
(368 -> 384, 24 -> 32, 16 -> 64, 8 output channels of a sub-pixel conv), against the oracle on the same seeded weights.
fp32 is bit-exact; fp16 is held to test_gpu_layers.compare's bounds against the fp16-storage oracle (the proxy adds only
exact moves to the layer kernels those bounds were measured for).  forward_with_cat equals torch.cat of to_cat and
forward(x) in the stated order, bit for bit.  Then the two aliasing patterns of the reference's cuda_inference.py:
combine_for_reading_2x(inplace=True) and restore_y_2x_with_cat_after.

The fp16 figures (max / rms, mean / rms per case) go to f16_ops_seam.json in subnet_utils' output directory (committed as
profiles/f16_ops_seam.json)."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import dcvc_oracle as O
import layer_utils as LU
import layout_ref as R
from subnet_utils import _OUT
from test_gpu_layers import F16_STATS, compare

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float16]

# cin, c, adaptor, shortcut, quant, H, W
DCB_CASES = [
    (256, 256, False, False, False, 5, 7),
    (368, 368, False, False, True, 3, 5),       # pad channels 368 .. 383
    (24, 16, True, False, False, 6, 10),        # cin_p 32, c_p 64
    (192, 368, True, True, True, 4, 6),
    (128, 128, False, True, False, 1, 9),
    (320, 320, False, False, False, 9, 9),
]
# cin, cout (before the shuffle), k, padding, H, W
SUBPEL_CASES = [
    (128, 4 * 32, 1, 0, 5, 6),
    (64, 4 * 8, 3, 1, 3, 4),                    # 8 output channels: below one pad unit
]


def _f16(dtype):
    return dtype == torch.float16


def _storage(a, f16):
    """the values a tensor of the model's dtype holds"""
    return O.Net._rh(a) if f16 else np.asarray(a, np.float32)


def cu(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda()


@pytest.fixture(scope="module", autouse=True)
def _record_f16_figures():
    yield
    seam = {k: dict(max_over_rms=v[0], mean_over_rms=v[1]) for k, v in F16_STATS.items() if k.startswith("seam ")}
    if seam:
        os.makedirs(_OUT, exist_ok=True)
        with open(os.path.join(_OUT, "f16_ops_seam.json"), "w") as f:
            json.dump(seam, f, indent=1, sort_keys=True)
            f.write("\n")


def _dcb_inputs(case, f16, hw=None):
    """(weights as the model's dtype holds them, x [1, cin, H, W], q [1, c, 1, 1] or None)"""
    cin, c, adaptor, shortcut, quant, H, W = case
    H, W = hw or (H, W)
    rng = np.random.default_rng(5000 + DCB_CASES.index(case))
    sd = {k: _storage(v, f16) for k, v in LU.make_dcb_weights(rng, "m", cin, c, adaptor).items()}
    q = _storage(rng.uniform(0.5, 1.5, (1, c, 1, 1)), f16) if quant else None
    x = _storage(np.random.default_rng(H * 100 + W).standard_normal((1, cin, H, W)), f16)
    return sd, x, q


@functools.lru_cache(maxsize=None)
def _dcb_ref(idx, f16, hw=None):
    """the oracle's value [1, c, H, W], computed once per case and type"""
    case = DCB_CASES[idx]
    sd, x, q = _dcb_inputs(case, f16, hw)
    net = O.Net(sd)
    y = (net.dcb_f16 if f16 else net.dcb)(O.nchw_to_hwc(x), "m", shortcut=case[3], q=None if q is None else q.reshape(-1))
    y = O.hwc_to_nchw(y)
    y.setflags(write=False)
    return y


def _dcb_proxy(case, sd, dtype):
    from opendcvc_amd import ops
    p = ops.DepthConvProxy()
    w = [cu(sd["m." + n], dtype) for n in LU.DCB_PROXY_PARAMS]
    if case[2]:
        p.set_param_with_adaptor(*w, cu(sd["m.adaptor.weight"], dtype), cu(sd["m.adaptor.bias"], dtype), case[3])
    else:
        p.set_param(*w, case[3])
    return p


def _to_cat_variants(n, H, W, dtype, seed):
    """to_cat of n channels: contiguous, a channel slice of a wider NCHW tensor (a view at a storage offset; for B == 1
    torch calls it contiguous) and a column slice of a wider one (strided rows)"""
    rng = np.random.default_rng(seed)
    wide_c = cu(rng.standard_normal((1, n + 5, H, W)), dtype)
    wide_w = cu(rng.standard_normal((1, n, H, W + 3)), dtype)
    strided = wide_w[..., 1:1 + W]
    assert not strided.is_contiguous()
    return [("contiguous", cu(rng.standard_normal((1, n, H, W)), dtype)), ("channel slice", wide_c[:, 2:2 + n]),
            ("column slice", strided)]


def _check_with_cat(proxy, x, out, what):
    H, W = out.shape[2:]
    for n in (3, out.shape[1]):
        for kind, to_cat in _to_cat_variants(n, H, W, out.dtype, n):
            before = to_cat.clone()
            for front in (True, False):
                got = proxy.forward_with_cat(x, to_cat, front)
                R.assert_cat(got, out, to_cat, front, f"{what}: forward_with_cat, {n} channels, {kind}, front={front}")
            assert torch.equal(to_cat, before), f"{what}: to_cat was changed"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("idx", range(len(DCB_CASES)), ids=[str(c) for c in DCB_CASES])
def test_depth_conv_proxy_nchw_vs_oracle(idx, dtype):
    case, f16 = DCB_CASES[idx], _f16(dtype)
    cin, c, adaptor, shortcut, quant, H, W = case
    sd, x, q = _dcb_inputs(case, f16)
    p = _dcb_proxy(case, sd, dtype)
    xd = cu(x, dtype)
    x_before = xd.clone()
    if quant:
        qd = cu(q, dtype)                                          # [1, C, 1, 1] in the model's own dtype
        out = p.forward_with_quant_step(xd, qd)
    else:
        out = p.forward(xd)
    torch.cuda.synchronize()
    assert out.shape == (1, c, H, W) and out.dtype == dtype and out.is_contiguous()
    assert torch.equal(xd, x_before), "the proxy changed its input"
    compare(out.float().cpu().numpy(), _dcb_ref(idx, f16), dtype, f"seam dcb {case}")
    if not quant:
        _check_with_cat(p, xd, out, f"dcb {case}")


@functools.lru_cache(maxsize=None)
def _subpel(idx, f16):
    cin, cout, k, pad, H, W = SUBPEL_CASES[idx]
    rng = np.random.default_rng(6000 + idx)
    sd = {n: _storage(v, f16) for n, v in LU.make_conv_weights(rng, "m", cout, cin, k).items()}
    x = _storage(rng.standard_normal((1, cin, H, W)), f16)
    net = O.Net(sd)
    y = (net.conv_f16 if f16 else net.conv)(O.nchw_to_hwc(x), "m", 1, pad)
    y = O.hwc_to_nchw(O.pixel_shuffle(y, 2))
    y.setflags(write=False)
    return sd, x, y


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("idx", range(len(SUBPEL_CASES)), ids=[str(c) for c in SUBPEL_CASES])
def test_subpel_proxy_nchw_vs_oracle(idx, dtype):
    from opendcvc_amd import ops
    cin, cout, k, pad, H, W = SUBPEL_CASES[idx]
    sd, x, ref = _subpel(idx, _f16(dtype))
    p = ops.SubpelConv2xProxy()
    p.set_param(cu(sd["m.weight"], dtype), cu(sd["m.bias"], dtype), pad)
    xd = cu(x, dtype)
    out = p.forward(xd)
    torch.cuda.synchronize()
    assert out.shape == (1, cout // 4, 2 * H, 2 * W) and out.dtype == dtype and out.is_contiguous()
    compare(out.float().cpu().numpy(), ref, dtype, f"seam subpel {SUBPEL_CASES[idx]}")
    _check_with_cat(p, xd, out, f"subpel {SUBPEL_CASES[idx]}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_proxy_reuse_across_map_sizes(dtype):
    """6 x 10, then 33 x 47 (the scratch grows, the small one is retired), then 6 x 10 again: the first and the third
    result are identical, and each is the oracle's"""
    idx, f16 = 2, _f16(dtype)
    case = DCB_CASES[idx]
    sd, x_small, _ = _dcb_inputs(case, f16)
    _, x_large, _ = _dcb_inputs(case, f16, (33, 47))
    p = _dcb_proxy(case, sd, dtype)
    xs, xl = cu(x_small, dtype), cu(x_large, dtype)
    first = p.forward(xs).clone()
    large = p.forward(xl).clone()
    third = p.forward(xs)
    torch.cuda.synchronize()
    R.assert_same_bits(third, first, "6 x 10 after 33 x 47")
    compare(first.float().cpu().numpy(), _dcb_ref(idx, f16), dtype, f"seam reuse 6x10 {case}")
    compare(large.float().cpu().numpy(), _dcb_ref(idx, f16, (33, 47)), dtype, f"seam reuse 33x47 {case}")


# ----------------------------------------------------------------------------- aliasing the reference relies on

def _np_dtype(dtype):
    return np.float16 if dtype == torch.float16 else np.float32


@pytest.mark.parametrize("dtype", DTYPES)
def test_combine_for_reading_2x_into_its_own_front_half(dtype):
    """cuda_inference.combine_for_reading_2x(x, mask, inplace=True): out = x[:, :C // 2]"""
    from opendcvc_amd import ops
    C, H, W = 8, 5, 7
    rng = np.random.default_rng(31)
    x = rng.standard_normal((1, C, H, W)).astype(_np_dtype(dtype))
    m = (rng.random((1, C, H, W)) > 0.5).astype(_np_dtype(dtype))
    xd, md = cu(x, dtype), cu(m, dtype)
    fresh = torch.empty((1, C // 2, H, W), dtype=dtype, device="cuda")
    ops.combine_for_reading_2x_cuda(fresh, xd, md)
    xm = x.astype(np.float32) * m.astype(np.float32)
    R.assert_same_bits(fresh, (xm[:, :C // 2] + xm[:, C // 2:]).astype(x.dtype), "out of place")
    R.assert_same_bits(xd, x, "x after the out-of-place call")
    out = xd[:, :C // 2]
    assert out.is_contiguous() and out.data_ptr() == xd.data_ptr()
    ops.combine_for_reading_2x_cuda(out, xd, md)
    torch.cuda.synchronize()
    R.assert_same_bits(xd[:, :C // 2], fresh, "in place")
    R.assert_same_bits(xd[:, C // 2:], x[:, C // 2:], "the back half of x")


@pytest.mark.parametrize("dtype", DTYPES)
def test_restore_y_2x_into_the_front_of_a_concat_buffer(dtype):
    """cuda_inference.restore_y_2x_with_cat_after: out = buf[:, :C1] of a [1, C1 + C2, H, W] buffer"""
    from opendcvc_amd import ops
    C1, C2, H, W = 8, 6, 5, 7
    rng = np.random.default_rng(32)
    nd = _np_dtype(dtype)
    y = rng.integers(-5, 6, (1, C1 // 2, H, W)).astype(nd)
    means = rng.standard_normal((1, C1, H, W)).astype(nd)
    m = (rng.random((1, C1, H, W)) > 0.5).astype(nd)
    yd, mud, md = cu(y, dtype), cu(means, dtype), cu(m, dtype)
    fresh = torch.empty((1, C1, H, W), dtype=dtype, device="cuda")
    ops.restore_y_2x_cuda(fresh, yd, mud, md)
    want = (np.concatenate([y, y], 1).astype(np.float32) + means.astype(np.float32)) * m.astype(np.float32)
    R.assert_same_bits(fresh, want.astype(nd), "into a fresh tensor")
    buf, raw = R.operand(None, (1, C1 + C2, H, W), dtype)          # every byte 0xFF: the sentinel
    out = buf[:, :C1]
    assert out.is_contiguous()
    ops.restore_y_2x_cuda(out, yd, mud, md)
    torch.cuda.synchronize()
    R.assert_same_bits(buf[:, :C1], fresh, "into the front of the wider buffer")
    assert R.still_ff(buf[:, C1:]), "the back part of the buffer was written"
    assert R.clean(raw, buf), "a byte outside the buffer was written"
    for t, a, name in ((yd, y, "y"), (mud, means, "means"), (md, m, "mask")):
        R.assert_same_bits(t, a, name + " after the calls")


@pytest.mark.parametrize("dtype", DTYPES)
def test_build_index_without_cond_out(dtype):
    """cuda_inference.build_index_dec / build_index_enc pass cond_out = None when there is no force_zero_thres (the
    reference's default): the indexes are the oracle's, the same as with a cond_out, and nothing else is written"""
    from opendcvc_amd import ops
    nd = _np_dtype(dtype)
    rng = np.random.default_rng(33)
    shape = (1, 8, 5, 7)
    scales = np.exp(rng.normal(-1, 2, shape))
    scales.flat[:6] = [0.0, 0.11, 0.12, 16.0, 40.0, 1e-4]
    scales = scales.astype(nd)
    sym = rng.integers(-128, 128, shape).astype(nd)
    args = (0.11, 16.0, O.LOG_SCALE_MIN, O.LOG_STEP_RECIP, 0.12)
    want = O.scale_to_index(np.clip(scales.astype(np.float32), np.float32(0.11), np.float32(16.0)), *args[:4])
    sd, symd = cu(scales, dtype), cu(sym, dtype)
    idx, raw_idx = R.operand(None, shape, torch.uint8)
    ops.build_index_dec_cuda(idx, None, sd, *args)
    pk, raw_pk = R.operand(None, shape, torch.int16)
    ops.build_index_enc_cuda(pk, None, symd, sd, *args)
    with_cond = torch.empty(shape, dtype=torch.uint8, device="cuda")
    ops.build_index_dec_cuda(with_cond, torch.empty(shape, dtype=torch.bool, device="cuda"), sd, *args)
    torch.cuda.synchronize()
    R.assert_same_bits(idx, want, "build_index_dec_cuda(cond_out=None)")
    R.assert_same_bits(idx, with_cond, "with and without cond_out")
    R.assert_same_bits(pk, (sym.astype(np.int32) * 256 + want).astype(np.int16), "build_index_enc_cuda(cond_out=None)")
    assert R.clean(raw_idx, idx) and R.clean(raw_pk, pk), "a byte outside the outputs was written"
    R.assert_same_bits(sd, scales, "scales after the calls")
