"""tests/layout_ref.py on the CPU: the numpy restatements of the layout kernels equal torch.nn.functional / permute, and the
comparison helpers of tests/test_gpu_ops_seam.py and tests/test_gpu_layout.py reject seeded mistakes (a test that cannot
fail checks nothing)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dcvc_oracle as O
import layer_utils as LU
import layout_ref as R

DTYPES = [np.float32, np.float16]


def _x(shape, dtype, seed=0):
    return np.random.default_rng(seed).standard_normal(shape).astype(dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C,H,W", [(1, 8, 8), (3, 16, 24), (9, 8, 16)])
def test_unshuffle8_and_shuffle8_equal_torch(dtype, C, H, W):
    x = _x((C, H, W), dtype)
    want = F.pixel_unshuffle(torch.from_numpy(x)[None], 8)[0].permute(1, 2, 0).contiguous().numpy()
    R.assert_same_bits(R.unshuffle8(x), want, "unshuffle8")
    R.assert_same_bits(R.unshuffle8(x), O.pixel_unshuffle(np.moveaxis(x, 0, 2), 8), "unshuffle8 vs the oracle")
    back = F.pixel_shuffle(torch.from_numpy(want).permute(2, 0, 1)[None], 8).numpy()
    R.assert_same_bits(R.shuffle8(want), back[0], "shuffle8")
    R.assert_same_bits(R.shuffle8(want), x, "shuffle8 inverts unshuffle8")
    R.assert_same_bits(R.shuffle8_nchw(R.hwc_to_nchw(want)), back, "shuffle8_nchw")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H,W", [(1, 1), (3, 5), (4, 33)])
@pytest.mark.parametrize("pads", [(0, 0), (3, 0), (0, 9), (3, 9)])
def test_replicate_pad_and_crop_equal_torch(dtype, H, W, pads):
    x = _x((H, W, 5), dtype)
    t = torch.from_numpy(x).permute(2, 0, 1)[None]
    want = F.pad(t.float(), (0, pads[1], 0, pads[0]), mode="replicate").to(t.dtype)
    R.assert_same_bits(R.replicate_pad_hwc(x, *pads), want[0].permute(1, 2, 0).contiguous().numpy(), "replicate_pad_hwc")
    R.assert_same_bits(R.replicate_pad_nchw(t.contiguous().numpy(), *pads), want.numpy(), "replicate_pad_nchw")
    padded = R.replicate_pad_hwc(x, *pads)
    R.assert_same_bits(R.crop_hwc(padded, H, W), x, "crop undoes the pad")
    R.assert_same_bits(R.crop_hwc(x, 1, W), torch.from_numpy(x)[:1, :W].contiguous().numpy(), "crop_hwc")


@pytest.mark.parametrize("dtype", DTYPES)
def test_layout_transposes_equal_permute(dtype):
    x = _x((1, 12, 3, 5), dtype)
    hwc = torch.from_numpy(x)[0].permute(1, 2, 0).contiguous().numpy()
    R.assert_same_bits(R.nchw_to_hwc(x), hwc, "nchw_to_hwc")
    R.assert_same_bits(R.hwc_to_nchw(hwc), x, "hwc_to_nchw")
    if dtype == np.float32:
        R.assert_same_bits(R.nchw_to_hwc(x), O.nchw_to_hwc(x), "nchw_to_hwc vs the oracle")


@pytest.mark.parametrize("dtype", DTYPES)
def test_bias_clamp_and_scale_equal_torch(dtype):
    x = (_x((4, 6, 64), dtype) * 2).astype(dtype)
    bias = _x(64, np.float32, 1)
    t, b = torch.from_numpy(x), torch.from_numpy(bias)
    want = (t.float() + b).to(t.dtype).float().clamp(0, 1).to(t.dtype).numpy()
    R.assert_same_bits(R.bias_clamp(x, bias, 1), want, "bias + clamp")
    R.assert_same_bits(R.bias_clamp(x, bias, 0), (t.float() + b).to(t.dtype).numpy(), "bias")
    R.assert_same_bits(R.bias_clamp(x, None, 0), x, "neither")
    one_rounding = np.clip(x.astype(np.float32) + bias, np.float32(0), np.float32(1)).astype(dtype)
    R.assert_same_bits(R.bias_clamp(x, bias, 1), one_rounding, "clamp in fp32, one rounding: the kernels' order")
    q = np.abs(_x(64, np.float32, 2)) + 0.5
    R.assert_same_bits(R.scale_channels(x, q), (t.float() * torch.from_numpy(q)).to(t.dtype).numpy(), "scale_channels")


# ----------------------------------------------------------------------------- the helpers reject seeded mistakes

def test_a_replicate_pad_that_repeats_the_wrong_row_is_rejected():
    x = _x((3, 5, 4), np.float32)
    wrong = np.concatenate([x, x[1:2], x[1:2]], axis=0)           # repeats row H - 2
    with pytest.raises(AssertionError, match="differ, first at \\[3, 0, 0\\]"):
        R.assert_same_bits(wrong, R.replicate_pad_hwc(x, 2, 0), "pad")
    R.assert_same_bits(np.concatenate([x, x[2:3], x[2:3]], axis=0), R.replicate_pad_hwc(x, 2, 0), "pad")


def test_bit_comparison_sees_what_equality_does_not():
    a = np.zeros(4, np.float16)
    b = a.copy()
    b[2] = -0.0
    assert np.array_equal(a, b)
    with pytest.raises(AssertionError, match="first at \\[2\\]"):
        R.assert_same_bits(a, b, "signed zero")
    with pytest.raises(AssertionError, match="dtype"):
        R.assert_same_bits(a, a.astype(np.float32), "dtype")
    with pytest.raises(AssertionError, match="shape"):
        R.assert_same_bits(a, a[:3], "shape")
    n = np.full(3, np.nan, np.float32)
    R.assert_same_bits(n, n.copy(), "the same NaN")


@pytest.mark.parametrize("front", [True, False])
def test_a_cat_in_the_wrong_order_is_rejected(front):
    out = torch.from_numpy(_x((1, 4, 3, 5), np.float16))
    wide = torch.from_numpy(_x((1, 9, 3, 5), np.float16, 1))
    to_cat = wide[:, 2:5]                                          # a channel-slice view
    good = torch.cat((to_cat, out), 1) if front else torch.cat((out, to_cat), 1)
    R.assert_cat(good, out, to_cat, front, "cat")
    with pytest.raises(AssertionError, match="differ"):
        R.assert_cat(good, out, to_cat, not front, "cat")
    with pytest.raises(AssertionError, match="not contiguous"):
        R.assert_cat(torch.cat((good, good), 3)[..., :5], out, to_cat, front, "cat")     # the right values, strided
    with pytest.raises(AssertionError, match="float32"):
        R.assert_cat(good.float(), out, to_cat, front, "cat")


def test_a_non_zero_pad_channel_is_rejected():
    x = torch.zeros((3, 5, 32), dtype=torch.float16)
    x[..., :24] = 1.5
    R.assert_pad_zero(x, 24, "pad")
    x[2, 4, 31] = 6e-8                                             # the smallest fp16 subnormal
    with pytest.raises(AssertionError, match="1 pad channel entries"):
        R.assert_pad_zero(x, 24, "pad")
    x[2, 4, 31] = -0.0                                             # compares equal to zero, is not the zero fill
    with pytest.raises(AssertionError, match="1 pad channel entries"):
        R.assert_pad_zero(x, 24, "pad")


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("ld,off", [(None, None), (20, 4), (13, 0), (13, 1), (16, 2)])
def test_a_write_one_element_past_c_in_a_guarded_view_is_seen(dtype, ld, off):
    """both kinds of operand(): layer_utils.guarded where its 16-byte rule fits, the raw-buffer view elsewhere"""
    C, es = 12, LU._es(dtype)
    if ld is None:
        ld, off = 32, 16 // es
    view, raw = R.operand(None, (3, 5, C), dtype, ld=ld, off=off, device="cpu")
    is_guarded = (ld * es) % 16 == 0 and (off * es) % 16 == 0
    assert view.stride() == (5 * ld, ld, 1) and (view.data_ptr() - raw.data_ptr()) % 16 == (off * es) % 16
    assert R.still_ff(view) and R.clean(raw, view)
    view.copy_(torch.ones((3, 5, C), dtype=dtype))                 # a kernel that writes its C channels and nothing else
    assert R.clean(raw, view) and not R.still_ff(view)
    if is_guarded:
        assert LU.untouched(raw, view)
    flat = raw.view(dtype)
    for where in (view.storage_offset() + 14 * ld + C,             # one element past C in the last pixel
                  view.storage_offset() + C,                       # ... in the first pixel (inside the map when ld == C)
                  view.storage_offset() - 1):                      # one element in front of the first
        if ld == C and where == view.storage_offset() + C:
            continue
        saved = flat[where].clone()
        flat[where] = 0
        assert not R.clean(raw, view), where
        if is_guarded:
            assert not LU.untouched(raw, view)
        flat[where] = saved
    assert R.clean(raw, view)


def test_operand_holds_its_values_and_nchw_shapes():
    vals = _x((1, 3, 4, 33), np.float16)
    view, raw = R.operand(vals, vals.shape, torch.float16, off=1, device="cpu")
    assert view.is_contiguous() and (view.data_ptr() - raw.data_ptr()) % 16 == 2
    R.assert_same_bits(view, vals, "values")
    assert R.clean(raw, view)
    hwc, raw = R.operand(vals[0, 0, :, :24].reshape(4, 3, 8), (4, 3, 8), torch.float16, ld=16, off=8, device="cpu")
    R.assert_same_bits(hwc, vals[0, 0, :, :24].reshape(4, 3, 8), "guarded values")
    assert LU.untouched(raw, hwc) and R.clean(raw, hwc)
