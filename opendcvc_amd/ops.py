"""Drop-in for the reference's operator module ``inference_extensions_cuda``
(src/layers/extensions/inference/bind.cpp:7-36, signatures def.h:6-107, import list
src/layers/cuda_inference.py:12-16): same function / class names, same argument order, torch
tensors in NCHW, B == 1, fp32 or fp16, outputs allocated by the callee unless an ``out`` argument
is given, in-place where the reference is in-place.  Registering this module under that name makes
the unmodified reference model code take its accelerated branch on ROCm (seam 2).

Every function launches HIP kernels of libdcvc_amd.so on torch's current stream; there is no
torch fallback.  The kernels index flat buffers, so every function first holds its tensors to the
seam's argument contract (seam 2: contiguous CUDA tensors of one floating-point
dtype, matching element counts, typed index outputs, B == 1 where the shape is read as
[1, C, H, W]) and raises DcvcError, naming the argument, before anything is launched.
"""
import torch

from . import _lib
from . import nn as L
from ._lib import DcvcError, check


_s = L._stream


_FLOATS = (torch.float16, torch.float32)


def _req(fn, floats, **others):
    """The seam's argument contract (seam 2), checked before anything is launched: every tensor is a
    contiguous CUDA tensor on one device, the floating-point ones (`floats`: name -> tensor, outputs included) share one
    of float16 / float32, and each of `others` (name=(tensor, allowed dtypes)) has one of its dtypes.  Returns the
    dtype code of the floating-point arguments."""
    first = None
    for name, t, allowed in [(n, t, _FLOATS) for n, t in floats.items()] + [(n, *v) for n, v in others.items()]:
        if not isinstance(t, torch.Tensor):
            raise DcvcError(f"{fn}: {name} must be a tensor, got {type(t).__name__}")
        if not t.is_cuda:
            raise DcvcError(f"{fn}: {name} must be a CUDA tensor, it is on {t.device}")
        if not t.is_contiguous():
            raise DcvcError(f"{fn}: {name} must be contiguous, got shape {tuple(t.shape)} strides {tuple(t.stride())}")
        if t.dtype not in allowed:
            raise DcvcError(f"{fn}: {name} is {t.dtype}, expected " + " or ".join(str(d) for d in allowed))
        if first is None:
            first = (name, t)
        elif t.device != first[1].device:
            raise DcvcError(f"{fn}: {name} is on {t.device}, {first[0]} is on {first[1].device}")
        if allowed is _FLOATS and t.dtype != first[1].dtype:
            raise DcvcError(f"{fn}: {name} is {t.dtype}, {first[0]} is {first[1].dtype}: one dtype per call")
    return L.dtype_code(first[1].dtype)


def _count(fn, name, t, n, why):
    if t.numel() != n:
        raise DcvcError(f"{fn}: {name} holds {t.numel()} elements (shape {tuple(t.shape)}), the kernel indexes {n} ({why})")


def _chw(fn, name, x, groups=1):
    """(C, H, W) of the [1, C, H, W] tensor x; C a multiple of `groups`"""
    if x.dim() != 4 or x.shape[0] != 1:
        raise DcvcError(f"{fn}: {name} must be [1, C, H, W] (B == 1), got {tuple(x.shape)}")
    if x.shape[1] % groups:
        raise DcvcError(f"{fn}: {name} has {x.shape[1]} channels, which do not divide into {groups} groups")
    return tuple(x.shape[1:])


def process_with_mask_cuda(y, scales, means, mask, force_zero_thres):
    fn = "process_with_mask_cuda"
    dt = _req(fn, dict(y=y, scales=scales, means=means, mask=mask))
    for name, t in (("scales", scales), ("means", means), ("mask", mask)):
        _count(fn, name, t, y.numel(), "as many as y")
    outs = [torch.empty_like(y) for _ in range(4)]
    check(_lib.lib().dcvc_op_process_with_mask(dt, L._p(y), L._p(scales), L._p(means), L._p(mask),
                                               float(force_zero_thres), *[L._p(o) for o in outs], y.numel(), _s()),
          "process_with_mask")
    return tuple(outs)   # y_res, y_q, y_hat, s_hat


def combine_for_reading_2x_cuda(out, x, mask):
    """out may be the front half x[:, :C // 2] of x itself (the reference's inplace=True): every element reads its two
    sources before it writes"""
    fn = "combine_for_reading_2x_cuda"
    dt = _req(fn, dict(x=x, mask=mask, out=out))
    _chw(fn, "x", x, 2)
    _count(fn, "mask", mask, x.numel(), "as many as x")
    _count(fn, "out", out, x.numel() // 2, "half of x")
    check(_lib.lib().dcvc_op_combine_for_reading_2x(dt, L._p(out), L._p(x), L._p(mask), x.numel() // 2, _s()),
          "combine_for_reading_2x")


def _restore(fn, groups, entry, out, y, means, mask):
    """out may be the front channel slice of a wider [1, C1 + C2, H, W] buffer (restore_y_2x_with_cat_after): for B == 1
    that slice is contiguous memory"""
    dt = _req(fn, dict(y=y, means=means, mask=mask, out=out))
    _chw(fn, "means", means, groups)
    _count(fn, "y", y, means.numel() // groups, f"1/{groups} of means")
    _count(fn, "mask", mask, means.numel(), "as many as means")
    _count(fn, "out", out, means.numel(), "as many as means")
    check(entry(dt, L._p(out), L._p(y), L._p(means), L._p(mask), y.numel(), _s()), fn[:-5])


def restore_y_2x_cuda(out, y, means, mask):
    _restore("restore_y_2x_cuda", 2, _lib.lib().dcvc_op_restore_y_2x, out, y, means, mask)


def restore_y_4x_cuda(out, y, means, mask):
    _restore("restore_y_4x_cuda", 4, _lib.lib().dcvc_op_restore_y_4x, out, y, means, mask)


def _index_args(fn, floats, out, out_dtype, cond_out):
    """_req and the counts of build_index_*: out of its own integer type, cond_out bool / uint8 or None (the reference
    passes None when there is no force_zero_thres: the kernel then writes no skip decisions), both as large as scales"""
    others = dict(out=(out, (out_dtype,)))
    if cond_out is not None:
        others["cond_out"] = (cond_out, (torch.bool, torch.uint8))
    dt = _req(fn, floats, **others)
    n = floats["scales"].numel()
    for name, t in ((k, v) for k, v in floats.items() if k != "scales"):
        _count(fn, name, t, n, "as many as scales")
    for name, (t, _) in others.items():
        _count(fn, name, t, n, "as many as scales")
    return dt


def build_index_dec_cuda(out, cond_out, scales, scale_min, scale_max, log_scale_min, log_step_recip, skip_thres):
    dt = _index_args("build_index_dec_cuda", dict(scales=scales), out, torch.uint8, cond_out)
    check(_lib.lib().dcvc_op_build_index_dec(dt, L._p(out), L._p(cond_out), L._p(scales), scale_min, scale_max,
                                             log_scale_min, log_step_recip, skip_thres, scales.numel(), _s()),
          "build_index_dec")


def build_index_enc_cuda(out, cond_out, symbols, scales, scale_min, scale_max, log_scale_min, log_step_recip,
                         skip_thres):
    dt = _index_args("build_index_enc_cuda", dict(scales=scales, symbols=symbols), out, torch.int16, cond_out)
    check(_lib.lib().dcvc_op_build_index_enc(dt, L._p(out), L._p(cond_out), L._p(symbols), L._p(scales), scale_min,
                                             scale_max, log_scale_min, log_step_recip, skip_thres, scales.numel(),
                                             _s()), "build_index_enc")


def round_and_to_int8_cuda(z):
    dt = _req("round_and_to_int8_cuda", dict(z=z))
    z8 = torch.empty(z.shape, dtype=torch.int8, device=z.device)
    check(_lib.lib().dcvc_op_round_and_to_int8(dt, L._p(z), L._p(z8), z.numel(), _s()), "round_and_to_int8")
    return z8


def clamp_reciprocal_with_quant_cuda(q_dec, y, min_val):
    fn = "clamp_reciprocal_with_quant_cuda"
    dt = _req(fn, dict(y=y, q_dec=q_dec))
    _count(fn, "q_dec", q_dec, y.numel(), "as many as y")
    q_out = torch.empty_like(q_dec)
    check(_lib.lib().dcvc_op_clamp_reciprocal_with_quant(dt, L._p(q_dec), L._p(y), float(min_val), L._p(q_out),
                                                         y.numel(), _s()), "clamp_reciprocal_with_quant")
    return q_out


def add_and_multiply_cuda(x0, x1, q):
    fn = "add_and_multiply_cuda"
    dt = _req(fn, dict(x0=x0, x1=x1, q=q))
    _count(fn, "x1", x1, x0.numel(), "as many as x0")
    _count(fn, "q", q, x0.numel(), "as many as x0")
    check(_lib.lib().dcvc_op_add_and_multiply(dt, L._p(x0), L._p(x1), L._p(q), x0.numel(), _s()), "add_and_multiply")


def bias_quant_cuda(x, bias, quant_step):
    fn = "bias_quant_cuda"
    dt = _req(fn, dict(x=x, bias=bias, quant_step=quant_step))
    C, H, W = _chw(fn, "x", x)
    _count(fn, "bias", bias, C, "one per channel of x")
    _count(fn, "quant_step", quant_step, C, "one per channel of x")
    check(_lib.lib().dcvc_op_bias_quant(dt, L._p(x), L._p(bias), L._p(quant_step), C, H * W, _s()), "bias_quant")


def bias_pixel_shuffle_8_cuda(out, x, bias, C, N, W, clamp):
    fn = "bias_pixel_shuffle_8_cuda"
    dt = _req(fn, dict(x=x, bias=bias, out=out))
    C, N, W = int(C), int(N), int(W)
    if C <= 0 or C % 64:
        raise DcvcError(f"{fn}: C = {C} must be a positive multiple of 64")
    if W <= 0 or N <= 0 or N % W:
        raise DcvcError(f"{fn}: N = {N} must be a positive multiple of W = {W}")
    _count(fn, "x", x, C * N, "C * N")
    _count(fn, "bias", bias, C, "C")
    if tuple(out.shape) != (1, C // 64, 8 * (N // W), 8 * W):
        raise DcvcError(f"{fn}: out must be {(1, C // 64, 8 * (N // W), 8 * W)}, got {tuple(out.shape)}")
    check(_lib.lib().dcvc_op_bias_pixel_shuffle_8(dt, L._p(out), L._p(x), L._p(bias), C, N // W, W,
                                                  int(bool(clamp)), _s()), "bias_pixel_shuffle_8")


def replicate_pad_cuda(x, padB, padR):
    fn = "replicate_pad_cuda"
    dt = _req(fn, dict(x=x))
    padB, padR = int(padB), int(padR)
    if x.dim() != 4 or x.numel() == 0:
        raise DcvcError(f"{fn}: x must be a non-empty [B, C, H, W] tensor, got {tuple(x.shape)}")
    if padB < 0 or padR < 0:
        raise DcvcError(f"{fn}: padB / padR must be >= 0, got {padB}, {padR}")
    B, C, H, W = x.shape
    out = torch.empty((B, C, H + padB, W + padR), dtype=x.dtype, device=x.device)
    check(_lib.lib().dcvc_op_replicate_pad(dt, L._p(x), B * C, H, W, padB, padR, L._p(out), _s()), "replicate_pad")
    return out


def bias_wsilu_depthwise_conv2d_cuda(x, weight, bias):
    fn = "bias_wsilu_depthwise_conv2d_cuda"
    dt = _req(fn, dict(x=x, weight=weight, bias=bias))
    C, H, W = _chw(fn, "x", x)
    _count(fn, "weight", weight, C * 9, "[C, 1, 3, 3]")
    _count(fn, "bias", bias, C, "one per channel of x")
    out = torch.empty_like(x)
    check(_lib.lib().dcvc_op_bias_wsilu_depthwise_conv2d(dt, L._p(x), L._p(weight), L._p(bias), C, H, W, L._p(out),
                                                         _s()), "bias_wsilu_depthwise_conv2d")
    return out


def _proxy_args(fn, x, cin, dtype, out_hw, quant_step=None, c=None, to_cat=None):
    """What a proxy's forward* takes, checked before anything is launched: x = [1, cin, H, W] of the layer's dtype on the
    GPU (a non-contiguous x is copied on the way to HWC), quant_step with one entry per output channel, to_cat a
    [1, C', Ho, Wo] tensor or view (torch.cat reads it through its strides) of the result's size out_hw(H, W)."""
    for name, t in (("x", x), ("quant_step", quant_step), ("to_cat", to_cat)):
        if t is None:
            continue
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.device != x.device:
            raise DcvcError(f"{fn}: {name} must be a CUDA tensor on x's device")
        if t.dtype != dtype:
            raise DcvcError(f"{fn}: {name} is {t.dtype}, the layer computes in {dtype}")
    if x.dim() != 4 or x.shape[0] != 1 or x.shape[1] != cin or x.numel() == 0:
        raise DcvcError(f"{fn}: x must be a non-empty [1, {cin}, H, W] tensor (B == 1), got {tuple(x.shape)}")
    if quant_step is not None:
        _count(fn, "quant_step", quant_step, c, "one per output channel")
    if to_cat is not None and (to_cat.dim() != 4 or (to_cat.shape[0], *to_cat.shape[2:]) != (1, *out_hw(*x.shape[2:]))):
        raise DcvcError(f"{fn}: to_cat must be [1, C, {', '.join(map(str, out_hw(*x.shape[2:])))}] (B == 1), got "
                        f"{tuple(to_cat.shape)}")


def _cat(out, to_cat, cat_at_front):
    return torch.cat((to_cat, out), dim=1) if cat_at_front else torch.cat((out, to_cat), dim=1)


class DepthConvProxy:
    """reference: DepthConvProxy (def.h:53-91, impl.cpp:7-121) - NCHW in / out around the fused block."""

    def __init__(self):
        self._blk = None
        self._c = None

    def _make(self, names, tensors, shortcut):
        sd = {"m." + n: t for n, t in zip(names, tensors)}
        self._blk = L.DepthConvBlock(sd, "m", tensors[0].dtype, shortcut=bool(shortcut))
        self._c = self._blk.c

    def set_param(self, dc_conv1_weight, dc_conv1_bias, dc_depth_conv_weight, dc_depth_conv_bias, dc_conv2_weight,
                  dc_conv2_bias, ffn_conv1_weight, ffn_conv1_bias, ffn_conv2_weight, ffn_conv2_bias, shortcut):
        names = ["dc.0.weight", "dc.0.bias", "dc.2.weight", "dc.2.bias", "dc.3.weight", "dc.3.bias", "ffn.0.weight",
                 "ffn.0.bias", "ffn.2.weight", "ffn.2.bias"]
        self._make(names, [dc_conv1_weight, dc_conv1_bias, dc_depth_conv_weight, dc_depth_conv_bias, dc_conv2_weight,
                           dc_conv2_bias, ffn_conv1_weight, ffn_conv1_bias, ffn_conv2_weight, ffn_conv2_bias], shortcut)

    def set_param_with_adaptor(self, dc_conv1_weight, dc_conv1_bias, dc_depth_conv_weight, dc_depth_conv_bias,
                               dc_conv2_weight, dc_conv2_bias, ffn_conv1_weight, ffn_conv1_bias, ffn_conv2_weight,
                               ffn_conv2_bias, adaptor_weight, adaptor_bias, shortcut):
        names = ["dc.0.weight", "dc.0.bias", "dc.2.weight", "dc.2.bias", "dc.3.weight", "dc.3.bias", "ffn.0.weight",
                 "ffn.0.bias", "ffn.2.weight", "ffn.2.bias", "adaptor.weight", "adaptor.bias"]
        self._make(names, [dc_conv1_weight, dc_conv1_bias, dc_depth_conv_weight, dc_depth_conv_bias, dc_conv2_weight,
                           dc_conv2_bias, ffn_conv1_weight, ffn_conv1_bias, ffn_conv2_weight, ffn_conv2_bias,
                           adaptor_weight, adaptor_bias], shortcut)

    def _run(self, fn, x, quant=None, to_cat=None):
        if self._blk is None:
            raise DcvcError("DepthConvProxy: set_param has not been called")
        _proxy_args("DepthConvProxy." + fn, x, self._blk.cin, self._blk.dtype, lambda H, W: (H, W), quant, self._c, to_cat)
        q = quant.reshape(-1).float().contiguous() if quant is not None else None
        return L.to_nchw(self._blk(L.to_hwc(x, self._blk.cin_p), quant=q), self._c)

    def forward(self, x):
        return self._run("forward", x)

    def forward_with_quant_step(self, x, quant_step):
        return self._run("forward_with_quant_step", x, quant_step)

    def forward_with_cat(self, x, to_cat, cat_at_front):
        return _cat(self._run("forward_with_cat", x, to_cat=to_cat), to_cat, cat_at_front)


class SubpelConv2xProxy:
    """reference: SubpelConv2xProxy (def.h:93-107, impl.cpp:123-167)"""

    def __init__(self):
        self._conv = None

    def set_param(self, weight, bias, padding):
        self._conv = L.Conv2d({"m.weight": weight, "m.bias": bias}, "m", weight.dtype, 1, int(padding),
                              _lib.EPI_SHUFFLE2)

    def _run(self, fn, x, to_cat=None):
        if self._conv is None:
            raise DcvcError("SubpelConv2xProxy: set_param has not been called")
        _proxy_args("SubpelConv2xProxy." + fn, x, self._conv.cin, self._conv.dtype, self._conv.out_hw, to_cat=to_cat)
        return L.to_nchw(self._conv(L.to_hwc(x, self._conv.cin_p)), self._conv.cout // 4)

    def forward(self, x):
        return self._run("forward", x)

    def forward_with_cat(self, x, to_cat, cat_at_front):
        return _cat(self._run("forward_with_cat", x, to_cat), to_cat, cat_at_front)
