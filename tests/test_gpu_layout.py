"""The layout kernels of csrc/dcvc_elem.hip, one by one through the C ABI, against their numpy restatements
(tests/layout_ref.py, held against torch on the CPU by tests/test_layout_ref_host.py).  They move data, or multiply once in
fp32 and round once, so every result is compared bit for bit, in both storage types.  Every operand lies in a 0xFF-filled
buffer (layer_utils.guarded where its 16-byte rule fits, the equivalent raw view elsewhere): a read outside an operand
brings a NaN into the result, a write outside it changes a byte that the test sees, and every source must come back
unchanged.  The shapes are the smallest that reach each form: one pixel, odd maps, more than one block (4 x 33 x 200),
channel counts that are no multiple of a vector, row strides above C, bases 2 / 4 / 8 bytes into the allocation, LDS
tiles at and above 64 KiB."""
import ctypes

import numpy as np
import pytest
import torch

import layer_utils as LU
import layout_ref as R

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float16]
MAPS = [(1, 1), (3, 5), (4, 33)]
CHANNELS = [3, 12, 64, 200]


def _np_dtype(dtype):
    return np.float16 if dtype == torch.float16 else np.float32


def _vals(shape, dtype, seed=0, scale=1.0):
    return (np.random.default_rng(seed).standard_normal(shape) * scale).astype(_np_dtype(dtype))


class Run:
    """The operands of one kernel call: src() / out() hand out views inside 0xFF-filled buffers, call() launches an entry
    on torch's current stream, done() checks that no byte outside an output changed and that every source is intact."""

    def __init__(self, dtype):
        from opendcvc_amd import nn
        self.dtype, self.dt = dtype, nn.dtype_code(dtype)
        self.srcs, self.outs = [], []

    def src(self, values, ld=None, off=0):
        view, raw = R.operand(values, values.shape, self.dtype, ld=ld, off=off)
        self.srcs.append((raw, raw.clone()))
        return view

    def vec(self, values_f32):
        v, raw = LU.guarded_vec(values_f32)
        self.srcs.append((raw, raw.clone()))
        return v

    def out(self, shape, ld=None, off=0):
        view, raw = R.operand(None, shape, self.dtype, ld=ld, off=off)
        self.outs.append((view, raw))
        return view

    @staticmethod
    def call(name, *args):
        from opendcvc_amd import _lib
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        _lib.check(getattr(_lib.lib(), name)(*args, st), name)

    def done(self):
        torch.cuda.synchronize()
        for view, raw in self.outs:
            assert R.clean(raw, view), "a byte outside the output changed"
        for raw, before in self.srcs:
            assert torch.equal(raw, before), "the call changed a source buffer"


def p(t):
    return ctypes.c_void_p(t.data_ptr())


# ----------------------------------------------------------------------------- NCHW <-> HWC

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("pad", [0, 8])
@pytest.mark.parametrize("C", CHANNELS)
@pytest.mark.parametrize("hw", MAPS)
def test_nchw_to_hwc(hw, C, pad, dtype):
    """ldo == C and ldo == C + 8: the kernel writes C channels per pixel and leaves the pad channels alone; nn.to_hwc
    hands the layers a map whose pad channels are zeros"""
    from opendcvc_amd import nn
    H, W = hw
    x = _vals((1, C, H, W), dtype, C + pad)
    r = Run(dtype)
    xd, out = r.src(x), r.out((H, W, C + pad))
    r.call("dcvc_nchw_to_hwc", r.dt, p(xd), C, H * W, p(out), C + pad)
    r.done()
    R.assert_same_bits(out[..., :C], R.nchw_to_hwc(x), "dcvc_nchw_to_hwc")
    assert R.still_ff(out[..., C:]), "the kernel wrote a pad channel"
    got = nn.to_hwc(xd, C + pad)
    torch.cuda.synchronize()
    assert got.shape == (H, W, C + pad) and got.dtype == dtype and got.is_contiguous()
    R.assert_same_bits(got[..., :C], R.nchw_to_hwc(x), "nn.to_hwc")
    R.assert_pad_zero(got, C, "nn.to_hwc")
    assert torch.equal(r.srcs[0][0], r.srcs[0][1])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", CHANNELS)
@pytest.mark.parametrize("hw", MAPS)
def test_hwc_to_nchw_from_a_channel_slice(hw, C, dtype):
    """the source is channels 5 .. 5 + C of a map C + 11 wide (ldx > C, non-zero channel offset)"""
    from opendcvc_amd import nn
    H, W = hw
    wide = _vals((H, W, C + 11), dtype, C)
    r = Run(dtype)
    x = r.src(wide)[..., 5:5 + C]
    out = r.out((1, C, H, W))
    r.call("dcvc_hwc_to_nchw", r.dt, p(x), C + 11, C, H * W, p(out))
    r.done()
    want = R.hwc_to_nchw(wide[..., 5:5 + C])
    R.assert_same_bits(out, want, "dcvc_hwc_to_nchw")
    got = nn.to_nchw(x, C)
    assert got.is_contiguous() and got.dtype == dtype
    R.assert_same_bits(got, want, "nn.to_nchw")


# ----------------------------------------------------------------------------- pad, crop, copy

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("extra", [0, 5])
@pytest.mark.parametrize("C", CHANNELS)
@pytest.mark.parametrize("pads", [(0, 0), (3, 0), (0, 9), (3, 9)])
@pytest.mark.parametrize("hw", MAPS)
def test_replicate_pad_hwc(hw, pads, C, extra, dtype):
    H, W = hw
    x = _vals((H, W, C), dtype, C + H)
    r = Run(dtype)
    xd = r.src(x, ld=C + extra)
    out = r.out((H + pads[0], W + pads[1], C), ld=C + (3 if extra else 0))
    r.call("dcvc_replicate_pad_hwc", r.dt, p(xd), xd.stride(1), H, W, C, pads[0], pads[1], p(out), out.stride(1))
    r.done()
    R.assert_same_bits(out, R.replicate_pad_hwc(x, *pads), "dcvc_replicate_pad_hwc")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("extra", [0, 5])
@pytest.mark.parametrize("C", CHANNELS)
@pytest.mark.parametrize("h2w2", [(3, 20), (2, 33), (1, 7), (4, 33)])
def test_crop_hwc(h2w2, C, extra, dtype):
    """W2 < W, W2 == W, H2 == 1 and the whole map, from 4 x 33"""
    H, W = 4, 33
    H2, W2 = h2w2
    x = _vals((H, W, C), dtype, C + H2)
    r = Run(dtype)
    xd = r.src(x, ld=C + extra)
    out = r.out((H2, W2, C), ld=C + (3 if extra else 0))
    r.call("dcvc_crop_hwc", r.dt, p(xd), xd.stride(1), W, H2, W2, C, p(out), out.stride(1))
    r.done()
    R.assert_same_bits(out, R.crop_hwc(x, H2, W2), "dcvc_crop_hwc")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", CHANNELS)
@pytest.mark.parametrize("hw", MAPS)
def test_copy_channels_slice_to_slice(hw, C, dtype):
    """channels 5 .. 5 + C of one map into channels 2 .. 2 + C of another: the other channels keep their sentinel"""
    H, W = hw
    wide = _vals((H, W, C + 11), dtype, C)
    r = Run(dtype)
    x = r.src(wide)[..., 5:5 + C]
    dst = r.out((H, W, C + 6))
    r.call("dcvc_copy_channels", r.dt, p(x), C + 11, H * W, C, p(dst[..., 2:]), C + 6)
    r.done()
    R.assert_same_bits(dst[..., 2:2 + C], wide[..., 5:5 + C], "dcvc_copy_channels")
    assert R.still_ff(dst[..., :2]) and R.still_ff(dst[..., 2 + C:]), "a channel outside the slice was written"


@pytest.mark.parametrize("n", [1, 1000])
def test_copy_f32(n):
    """the source goes on with finite numbers behind n (behind a 0xFF guard, a copy of one entry too many would write
    0xFF over 0xFF and show nowhere); the destination's entries behind n are outside the view"""
    vals = np.random.default_rng(n).standard_normal(n + 8).astype(np.float32)
    r = Run(torch.float32)
    src = r.src(vals)
    dst = r.out((n,))
    r.call("dcvc_copy_f32", p(dst), p(src), n)
    r.done()
    R.assert_same_bits(dst, vals[:n], "dcvc_copy_f32")


# ----------------------------------------------------------------------------- scale_channels

def _scale(dtype, hw, C, ldx, ldo, offx, offo, seed=7):
    H, W = hw
    x = _vals((H, W, C), dtype, seed, 3.0)
    q = np.random.default_rng(seed + 1).uniform(0.3, 2.5, C).astype(np.float32)
    r = Run(dtype)
    xd, qd = r.src(x, ld=ldx, off=offx), r.vec(q)
    out = r.out((H, W, C), ld=ldo, off=offo)
    r.call("dcvc_scale_channels", r.dt, p(xd), ldx, p(qd), H * W, C, p(out), ldo)
    r.done()
    R.assert_same_bits(out, R.scale_channels(x, q), f"dcvc_scale_channels C={C} ld=({ldx}, {ldo}) off=({offx}, {offo})")
    return R.to_np(out)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hw", MAPS)
def test_scale_channels_both_forms(hw, dtype):
    """the expected value is (x.float() * q).to(dtype).  Vector form: C = 64, 16-byte aligned bases, row strides a multiple
    of the vector.  Scalar form: a base one element (2 / 4 bytes) into the allocation on either side, and a row stride that
    is no multiple of the vector; on the operands that qualify for both, the two forms agree bit for bit."""
    vec = _scale(dtype, hw, 64, 64, 64, 0, 0)
    for ldx, ldo, offx, offo in ((64, 64, 1, 0), (64, 64, 0, 1), (72, 72, 1, 1), (66, 64, 0, 0), (64, 66, 0, 0)):
        R.assert_same_bits(_scale(dtype, hw, 64, ldx, ldo, offx, offo), vec, "scalar form vs vector form")
    R.assert_same_bits(_scale(dtype, hw, 64, 72, 80, 0, 0), vec, "vector form, row strides above C")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", [3, 12, 200])
@pytest.mark.parametrize("hw", MAPS)
def test_scale_channels_odd_widths(hw, C, dtype):
    """C = 12 is a whole number of vectors in fp32 and not in fp16; 3 in neither; 200 in both (more than one block)"""
    _scale(dtype, hw, C, C, C, 0, 0)
    _scale(dtype, hw, C, C + 5, C + 3, 0, 0)


# ----------------------------------------------------------------------------- pixel (un)shuffle by 8

def _s8_cases():
    """(name, C per dtype, H, W, base offset in bytes): the tiled form needs 16-byte aligned bases and an LDS tile of
    C * 8 rows * 256 columns <= 64 KiB; everything else takes the untiled form"""
    return [("tiled", {4: 3, 2: 3}, 16, 24, 0),
            ("base 8 bytes in", {4: 3, 2: 3}, 16, 24, 8),
            ("tile of exactly 64 KiB", {4: 8, 2: 16}, 8, 16, 0),
            ("tile above 64 KiB", {4: 9, 2: 17}, 8, 16, 0),
            ("two segments, the second ragged", {4: 1, 2: 1}, 8, 264, 0)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("wide", [False, True], ids=["tight", "wide"])
@pytest.mark.parametrize("case", _s8_cases(), ids=lambda c: c[0])
def test_unshuffle8(case, wide, dtype):
    """wide: ldo > 64 C, into channels 16 .. of a wider map whose other channels keep their sentinel"""
    _, Cs, H, W, off_bytes = case
    es = LU._es(dtype)
    C, off = Cs[es], off_bytes // es
    x = _vals((1, C, H, W), dtype, C)
    r = Run(dtype)
    xd = r.src(x, off=off)
    cw = 64 * C + (32 if wide else 0)
    full = r.out((H // 8, W // 8, cw), off=off)
    out = full[..., 16:16 + 64 * C] if wide else full
    r.call("dcvc_unshuffle8", r.dt, p(xd), C, H, W, p(out), cw)
    r.done()
    want = R.unshuffle8(x[0])
    R.assert_same_bits(out, want, "dcvc_unshuffle8")
    R.assert_same_bits(out, torch.nn.functional.pixel_unshuffle(torch.from_numpy(x), 8)[0].permute(1, 2, 0).contiguous(),
                       "dcvc_unshuffle8 vs F.pixel_unshuffle")
    if wide:
        assert R.still_ff(full[..., :16]) and R.still_ff(full[..., 16 + 64 * C:]), "a channel outside the slice was written"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("bias,clamp", [(True, 1), (False, 1), (True, 0), (False, 0)],
                         ids=["bias+clamp", "clamp", "bias", "move"])
@pytest.mark.parametrize("wide", [False, True], ids=["tight", "wide"])
@pytest.mark.parametrize("case", _s8_cases(), ids=lambda c: c[0])
def test_shuffle8_clamp(case, wide, bias, clamp, dtype):
    """values from about -3 to 4: without the clamp they must come through unchanged.  wide: ld > 64 C, the source is
    channels 16 .. of a wider map"""
    _, Cs, H, W, off_bytes = case
    es = LU._es(dtype)
    C, off = Cs[es], off_bytes // es
    cw = 64 * C + (32 if wide else 0)
    src = _vals((H // 8, W // 8, cw), dtype, C + clamp, 1.5) + _np_dtype(dtype)(0.5)
    b = np.random.default_rng(C).uniform(-0.5, 0.5, 64 * C).astype(np.float32) if bias else None
    r = Run(dtype)
    full = r.src(src, off=off)
    x = full[..., 16:16 + 64 * C] if wide else full
    bd = r.vec(b) if bias else None
    out = r.out((1, C, H, W), off=off)
    r.call("dcvc_shuffle8_clamp", r.dt, p(x), cw, p(bd) if bias else None, C, H // 8, W // 8, clamp, p(out))
    r.done()
    xs = src[..., 16:16 + 64 * C] if wide else src
    if not clamp:
        assert xs.min() < -1 and xs.max() > 2
    want = R.bias_clamp(xs, b, clamp)
    R.assert_same_bits(out[0], R.shuffle8(want), "dcvc_shuffle8_clamp")
    R.assert_same_bits(out, torch.nn.functional.pixel_shuffle(torch.from_numpy(want).permute(2, 0, 1)[None], 8),
                       "dcvc_shuffle8_clamp vs F.pixel_shuffle")


# ----------------------------------------------------------------------------- the seam's NCHW forms, both types

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("clamp", [True, False])
@pytest.mark.parametrize("C,H,W", [(64, 1, 1), (192, 2, 3), (128, 3, 5)])
def test_op_bias_pixel_shuffle_8(C, H, W, clamp, dtype):
    from opendcvc_amd import ops
    x = _vals((1, C, H, W), dtype, C, 1.5)
    b = _vals((C,), dtype, C + 1, 0.5)
    r = Run(dtype)
    xd, bd = r.src(x), r.src(b)
    out = r.out((1, C // 64, 8 * H, 8 * W))
    ops.bias_pixel_shuffle_8_cuda(out, xd, bd, C, H * W, W, clamp)
    r.done()
    want = R.shuffle8(R.bias_clamp(R.nchw_to_hwc(x), b.astype(np.float32), clamp))[None]
    R.assert_same_bits(out, want, "bias_pixel_shuffle_8_cuda")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("pads", [(0, 0), (3, 0), (0, 9), (3, 9)])
@pytest.mark.parametrize("shape", [(1, 3, 1, 1), (2, 3, 3, 5), (1, 2, 4, 33)])
def test_op_replicate_pad(shape, pads, dtype):
    """B = 2 included: the entry pads B * C planes"""
    from opendcvc_amd import ops
    x = _vals(shape, dtype, shape[2])
    r = Run(dtype)
    xd = r.src(x)
    got = ops.replicate_pad_cuda(xd, *pads)
    r.done()
    assert got.is_contiguous() and got.dtype == dtype
    R.assert_same_bits(got, R.replicate_pad_nchw(x, *pads), "replicate_pad_cuda")
