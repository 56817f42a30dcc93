"""The operator seam's argument contract (seam 2): opendcvc_amd.ops refuses a call whose tensors the
kernel would index out of bounds or read in the wrong type - mixed float16 / float32, a CPU or strided tensor, an element
count that does not match, a wrong index dtype, B > 1 where the shape is read as [1, C, H, W], channels that do not
divide into the groups - with a DcvcError that begins with the function's and the offending argument's name, BEFORE
anything is launched.  Such a call must never reach the library, so these tests run with opendcvc_amd._lib.lib replaced
by a stand-in that records every entry it is asked for and launches nothing: a refused call records nothing, the valid
control call of each function records exactly its one entry.  (Real CUDA tensors of a few elements: the checks look at
devices, strides and dtypes.)"""
import inspect
import re

import numpy as np
import pytest
import torch

import dcvc_oracle as O
import layer_utils as LU

gpu = pytest.mark.gpu


class Recorder:
    """Stand-in for the loaded library: any attribute is a callable that records its name and returns 0.  (Handles of
    layer objects that happen to be collected meanwhile still go to the real library, unrecorded.)"""

    def __init__(self, real):
        self._real, self.calls = real, []

    def __getattr__(self, name):
        if name.endswith("_destroy"):
            return getattr(self._real, name)

        def entry(*args):
            self.calls.append(name)
            return 0
        return entry


@pytest.fixture
def rec(monkeypatch):
    from opendcvc_amd import _lib
    r = Recorder(_lib.lib())
    monkeypatch.setattr(_lib, "lib", lambda: r)
    return r


def T(*shape, dtype=torch.float32):
    return torch.zeros(shape, dtype=dtype, device="cuda")


class Spec:
    """a tensor argument of a valid call, described without allocating it (the table is read while tests are collected)"""

    def __init__(self, *shape, dtype=torch.float32):
        self.shape, self.dtype = shape, dtype

    @property
    def is_float(self):
        return self.dtype.is_floating_point


S = (1, 4, 2, 3)
IDX = dict(scale_min=0.11, scale_max=16.0, log_scale_min=O.LOG_SCALE_MIN, log_step_recip=O.LOG_STEP_RECIP, skip_thres=0.12)

# function -> its valid call (keyword arguments in the function's own names)
VALID = {
    "process_with_mask_cuda": dict(y=Spec(*S), scales=Spec(*S), means=Spec(*S), mask=Spec(*S), force_zero_thres=0.12),
    "combine_for_reading_2x_cuda": dict(out=Spec(1, 2, 2, 3), x=Spec(*S), mask=Spec(*S)),
    "restore_y_2x_cuda": dict(out=Spec(*S), y=Spec(1, 2, 2, 3), means=Spec(*S), mask=Spec(*S)),
    "restore_y_4x_cuda": dict(out=Spec(*S), y=Spec(1, 1, 2, 3), means=Spec(*S), mask=Spec(*S)),
    "build_index_dec_cuda": dict(out=Spec(*S, dtype=torch.uint8), cond_out=Spec(*S, dtype=torch.bool), scales=Spec(*S), **IDX),
    "build_index_enc_cuda": dict(out=Spec(*S, dtype=torch.int16), cond_out=Spec(*S, dtype=torch.bool), symbols=Spec(*S),
                                 scales=Spec(*S), **IDX),
    "round_and_to_int8_cuda": dict(z=Spec(*S)),
    "clamp_reciprocal_with_quant_cuda": dict(q_dec=Spec(*S), y=Spec(*S), min_val=0.5),
    "add_and_multiply_cuda": dict(x0=Spec(*S), x1=Spec(*S), q=Spec(*S)),
    "bias_quant_cuda": dict(x=Spec(*S), bias=Spec(4), quant_step=Spec(1, 4, 1, 1)),
    "bias_pixel_shuffle_8_cuda": dict(out=Spec(1, 1, 8, 16), x=Spec(1, 64, 1, 2), bias=Spec(64), C=64, N=2, W=2, clamp=True),
    "replicate_pad_cuda": dict(x=Spec(2, 3, 2, 3), padB=1, padR=2),
    "bias_wsilu_depthwise_conv2d_cuda": dict(x=Spec(*S), weight=Spec(4, 1, 3, 3), bias=Spec(4)),
}
# the argument whose size the others are held to: growing it is reported against them (rows of their own)
ANCHOR = {"process_with_mask_cuda": "y", "combine_for_reading_2x_cuda": "x", "restore_y_2x_cuda": "means",
          "restore_y_4x_cuda": "means", "build_index_dec_cuda": "scales", "build_index_enc_cuda": "scales",
          "round_and_to_int8_cuda": "z", "clamp_reciprocal_with_quant_cuda": "y", "add_and_multiply_cuda": "x0",
          "bias_quant_cuda": "x", "replicate_pad_cuda": "x", "bias_wsilu_depthwise_conv2d_cuda": "x"}
# the floating-point tensor whose dtype the others are held to, and the one checked right after it: a call in which only
# the first has the other float type is reported against the second
FIRST_FLOATS = {"process_with_mask_cuda": ("y", "scales"), "combine_for_reading_2x_cuda": ("x", "mask"),
                "restore_y_2x_cuda": ("y", "means"), "restore_y_4x_cuda": ("y", "means"),
                "build_index_enc_cuda": ("scales", "symbols"), "clamp_reciprocal_with_quant_cuda": ("y", "q_dec"),
                "add_and_multiply_cuda": ("x0", "x1"), "bias_quant_cuda": ("x", "bias"),
                "bias_pixel_shuffle_8_cuda": ("x", "bias"), "bias_wsilu_depthwise_conv2d_cuda": ("x", "weight")}


def valid(fn):
    """the valid call's arguments, its tensors allocated on the GPU"""
    return {k: T(*v.shape, dtype=v.dtype) if isinstance(v, Spec) else v for k, v in VALID[fn].items()}


def _strided(t):
    wide = torch.zeros((*t.shape[:-1], 2 * t.shape[-1]), dtype=t.dtype, device=t.device)[..., ::2]
    assert wide.shape == t.shape and not wide.is_contiguous()
    return wide


MUTATIONS = {
    "other float type": lambda t: t.half(),
    "float64": lambda t: t.double(),
    "wrong index type": lambda t: t.to(torch.int32),
    "on the CPU": lambda t: t.cpu(),
    "strided": _strided,
    "one column more": lambda t: torch.zeros((*t.shape[:-1], t.shape[-1] + 1), dtype=t.dtype, device=t.device),
    "B = 2": lambda t: torch.cat((t, t), 0),
    "not a tensor": lambda t: 1.0,
}


def _rows():
    """(function, mutated argument, mutation, the argument the message must name)"""
    rows = []
    for fn, args in VALID.items():
        for arg, v in args.items():
            if not isinstance(v, Spec):
                continue
            kinds = ["on the CPU", "strided", "not a tensor"]
            if not v.is_float:
                kinds += ["wrong index type", "other float type"]
            else:                       # the only floating-point tensor of a call may be of either type
                kinds += ["float64"] + (["other float type"] if fn in FIRST_FLOATS else [])
            if arg != ANCHOR.get(fn):
                kinds.append("one column more")
            for k in kinds:
                first, second = FIRST_FLOATS.get(fn, (None, None))
                rows.append((fn, arg, k, second if (k == "other float type" and arg == first) else arg))
    # the shape is read as [1, C, H, W]: B = 2 is refused (a bigger x alone: the first complaint is about x / means)
    rows += [(fn, ANCHOR[fn], "B = 2", ANCHOR[fn]) for fn in ("combine_for_reading_2x_cuda", "restore_y_2x_cuda",
                                                             "restore_y_4x_cuda", "bias_quant_cuda",
                                                             "bias_wsilu_depthwise_conv2d_cuda")]
    return rows


# (function, overrides of the valid call, the argument the message must name): what no single mutation reaches
SPECIAL = [
    ("combine_for_reading_2x_cuda", lambda: dict(out=T(1, 1, 2, 3), x=T(1, 3, 2, 3), mask=T(1, 3, 2, 3)), "x"),      # 3 channels, 2 groups
    ("restore_y_2x_cuda", lambda: dict(out=T(1, 3, 2, 3), y=T(1, 1, 2, 3), means=T(1, 3, 2, 3), mask=T(1, 3, 2, 3)), "means"),
    ("restore_y_4x_cuda", lambda: dict(out=T(1, 6, 2, 3), y=T(1, 1, 2, 3), means=T(1, 6, 2, 3), mask=T(1, 6, 2, 3)), "means"),
    ("restore_y_2x_cuda", lambda: dict(y=T(1, 4, 2, 3)), "y"),                      # y as large as means: out would hold 2 x
    ("restore_y_4x_cuda", lambda: dict(y=T(1, 2, 2, 3)), "y"),                      # the 2x call's y
    ("combine_for_reading_2x_cuda", lambda: dict(out=T(*S)), "out"),                # out as large as x
    ("bias_pixel_shuffle_8_cuda", lambda: dict(out=T(1, 1, 16, 8)), "out"),         # the right count, the wrong shape
    ("bias_pixel_shuffle_8_cuda", lambda: dict(C=32, x=T(1, 32, 1, 2), bias=T(32)), "C"),
    ("bias_pixel_shuffle_8_cuda", lambda: dict(N=3, x=T(1, 64, 1, 3)), "N"),
    ("bias_pixel_shuffle_8_cuda", lambda: dict(C=128), "x"),                        # C the tensor does not hold
    ("replicate_pad_cuda", lambda: dict(x=T(3, 2, 3)), "x"),
    ("replicate_pad_cuda", lambda: dict(padB=-1), "padB"),
    ("replicate_pad_cuda", lambda: dict(x=T(2, 3, 0, 3)), "x"),
    ("build_index_dec_cuda", lambda: dict(out=T(*S, dtype=torch.int16)), "out"),     # the encoder's packed type
    ("build_index_enc_cuda", lambda: dict(out=T(*S, dtype=torch.uint8)), "out"),     # the decoder's index type
    ("build_index_dec_cuda", lambda: dict(cond_out=T(*S, dtype=torch.int16)), "cond_out"),
    ("bias_quant_cuda", lambda: dict(quant_step=T(1, 1, 1, 1)), "quant_step"),       # a scalar step
    ("bias_quant_cuda", lambda: dict(bias=T(8)), "bias"),
]


def _entry(fn):
    return "dcvc_op_" + fn[:-len("_cuda")]


def _refused(fn, named):
    """the message states the offending argument first: '<function>: <argument> ...'"""
    from opendcvc_amd._lib import DcvcError
    return pytest.raises(DcvcError, match=rf"^{re.escape(fn)}: {named}\b")


def test_the_table_covers_every_tensor_argument_of_every_function():
    """(needs no GPU: the table and the signatures)"""
    from opendcvc_amd import ops
    public = {n for n, f in inspect.getmembers(ops, inspect.isfunction) if not n.startswith("_") and f.__module__ == ops.__name__}
    assert public == set(VALID), public ^ set(VALID)
    rows = _rows()
    for fn, args in VALID.items():
        assert list(args) == list(inspect.signature(getattr(ops, fn)).parameters), fn
        floats = [a for a, v in args.items() if isinstance(v, Spec) and v.is_float]
        assert (fn in FIRST_FLOATS) == (len(floats) > 1) and set(FIRST_FLOATS.get(fn, ())) <= set(floats), fn
        for arg, v in args.items():
            if isinstance(v, Spec):
                kinds = {k for f, a, k, _ in rows if (f, a) == (fn, arg)}
                assert {"on the CPU", "strided", "not a tensor"} <= kinds, (fn, arg, kinds)
                assert "other float type" in kinds or (v.is_float and len(floats) == 1), (fn, arg, kinds)
                assert "float64" in kinds or "wrong index type" in kinds, (fn, arg, kinds)
                assert "one column more" in kinds or arg == ANCHOR[fn], (fn, arg)


@gpu
@pytest.mark.parametrize("fn", list(VALID))
def test_a_valid_call_reaches_its_entry_exactly_once(rec, fn):
    from opendcvc_amd import ops
    getattr(ops, fn)(**valid(fn))
    assert rec.calls == [_entry(fn)]
    half = {k: v.half() if isinstance(v, torch.Tensor) and v.is_floating_point() else v for k, v in valid(fn).items()}
    getattr(ops, fn)(**half)
    assert rec.calls == [_entry(fn)] * 2


@gpu
@pytest.mark.parametrize("fn", ["build_index_dec_cuda", "build_index_enc_cuda"])
def test_build_index_without_cond_out_reaches_its_entry_exactly_once(rec, fn):
    """cond_out is optional (the reference passes None when there is no force_zero_thres)"""
    from opendcvc_amd import ops
    getattr(ops, fn)(**{**valid(fn), "cond_out": None})
    assert rec.calls == [_entry(fn)]


@gpu
@pytest.mark.parametrize("fn,arg,kind,named", _rows(), ids=lambda v: v if isinstance(v, str) else None)
def test_a_bad_tensor_argument_is_refused_before_any_launch(rec, fn, arg, kind, named):
    """('not a tensor' is a number in the argument's place: cond_out may be None, nothing else)"""
    from opendcvc_amd import ops
    args = valid(fn)
    args[arg] = MUTATIONS[kind](args[arg])
    with _refused(fn, named):
        getattr(ops, fn)(**args)
    assert rec.calls == []


@gpu
@pytest.mark.parametrize("fn,override,named", SPECIAL, ids=[f"{f}-{n}-{i}" for i, (f, _, n) in enumerate(SPECIAL)])
def test_a_call_the_kernel_would_misindex_is_refused_before_any_launch(rec, fn, override, named):
    from opendcvc_amd import ops
    args = {**valid(fn), **override()}
    with _refused(fn, named):
        getattr(ops, fn)(**args)
    assert rec.calls == []


# ----------------------------------------------------------------------------- the proxies

DCB_ENTRIES = ["dcvc_nchw_to_hwc", "dcvc_dcb_scratch_bytes", "dcvc_dcb_forward_chained", "dcvc_hwc_to_nchw"]
CONV_ENTRIES = ["dcvc_nchw_to_hwc", "dcvc_conv_forward_scaled", "dcvc_hwc_to_nchw"]


@pytest.fixture(scope="module")
def proxies():
    """built with the real library, before a test swaps it: a block 24 -> 16 with adaptor and a sub-pixel conv 16 -> 4 x 8"""
    from opendcvc_amd import ops
    rng = np.random.default_rng(1)
    cu = lambda a: torch.from_numpy(a).cuda()
    sd = LU.make_dcb_weights(rng, "m", 24, 16, True)
    dcb = ops.DepthConvProxy()
    dcb.set_param_with_adaptor(*[cu(sd["m." + n]) for n in LU.DCB_PROXY_PARAMS], cu(sd["m.adaptor.weight"]),
                               cu(sd["m.adaptor.bias"]), False)
    w = LU.make_conv_weights(rng, "m", 32, 16, 3)
    sub = ops.SubpelConv2xProxy()
    sub.set_param(cu(w["m.weight"]), cu(w["m.bias"]), 1)
    return dcb, sub


@gpu
def test_valid_proxy_calls_reach_their_entries(rec, proxies):
    dcb, sub = proxies
    x = T(1, 24, 2, 3)
    assert dcb.forward(x).shape == (1, 16, 2, 3) and rec.calls == DCB_ENTRIES
    assert dcb.forward_with_quant_step(x, T(1, 16, 1, 1)).shape == (1, 16, 2, 3) and rec.calls == DCB_ENTRIES * 2
    assert dcb.forward_with_cat(x, T(1, 5, 2, 3), True).shape == (1, 21, 2, 3) and rec.calls == DCB_ENTRIES * 3
    del rec.calls[:]
    x = T(1, 16, 2, 3)
    assert sub.forward(x).shape == (1, 8, 4, 6) and rec.calls == CONV_ENTRIES
    assert sub.forward_with_cat(x, T(1, 5, 4, 6), False).shape == (1, 13, 4, 6) and rec.calls == CONV_ENTRIES * 2


PROXY_BAD = [
    # proxy, method, arguments, the argument the message must name
    ("dcb", "forward", lambda: (T(2, 24, 2, 3),), "x"),                                   # B = 2
    ("dcb", "forward", lambda: (T(1, 16, 2, 3),), "x"),                                   # c instead of cin channels
    ("dcb", "forward", lambda: (T(1, 40, 2, 3),), "x"),                                   # more than cin_p channels
    ("dcb", "forward", lambda: (T(24, 2, 3),), "x"),
    ("dcb", "forward", lambda: (T(1, 24, 0, 3),), "x"),
    ("dcb", "forward", lambda: (T(1, 24, 2, 3).half(),), "x"),                            # an fp32 block
    ("dcb", "forward", lambda: (T(1, 24, 2, 3).cpu(),), "x"),
    ("dcb", "forward_with_quant_step", lambda: (T(2, 24, 2, 3), T(1, 16, 1, 1)), "x"),
    ("dcb", "forward_with_quant_step", lambda: (T(1, 24, 2, 3), T(1, 24, 1, 1)), "quant_step"),   # cin entries
    ("dcb", "forward_with_quant_step", lambda: (T(1, 24, 2, 3), T(1, 1, 1, 1)), "quant_step"),
    ("dcb", "forward_with_quant_step", lambda: (T(1, 24, 2, 3), T(1, 16, 1, 1).half()), "quant_step"),
    ("dcb", "forward_with_quant_step", lambda: (T(1, 24, 2, 3), T(1, 16, 1, 1).cpu()), "quant_step"),
    ("dcb", "forward_with_cat", lambda: (T(2, 24, 2, 3), T(2, 5, 2, 3), True), "x"),
    ("dcb", "forward_with_cat", lambda: (T(1, 24, 2, 3), T(2, 5, 2, 3), True), "to_cat"),
    ("dcb", "forward_with_cat", lambda: (T(1, 24, 2, 3), T(1, 5, 3, 3), False), "to_cat"),
    ("dcb", "forward_with_cat", lambda: (T(1, 24, 2, 3), T(1, 5, 2, 3).half(), True), "to_cat"),
    ("dcb", "forward_with_cat", lambda: (T(1, 24, 2, 3), T(1, 5, 2, 3).cpu(), True), "to_cat"),
    ("sub", "forward", lambda: (T(2, 16, 2, 3),), "x"),
    ("sub", "forward", lambda: (T(1, 8, 2, 3),), "x"),
    ("sub", "forward", lambda: (T(1, 16, 2, 3).half(),), "x"),
    ("sub", "forward", lambda: (T(1, 16, 2, 3).cpu(),), "x"),
    ("sub", "forward_with_cat", lambda: (T(2, 16, 2, 3), T(2, 5, 4, 6), True), "x"),
    ("sub", "forward_with_cat", lambda: (T(1, 16, 2, 3), T(1, 5, 2, 3), True), "to_cat"),  # x's size, not the result's
    ("sub", "forward_with_cat", lambda: (T(1, 16, 2, 3), T(1, 5, 4, 6).half(), False), "to_cat"),
]


@gpu
@pytest.mark.parametrize("which,method,make,named", PROXY_BAD, ids=[f"{w}.{m}-{n}-{i}" for i, (w, m, _, n) in enumerate(PROXY_BAD)])
def test_a_bad_proxy_call_is_refused_before_any_launch(rec, proxies, which, method, make, named):
    proxy, cls = (proxies[0], "DepthConvProxy") if which == "dcb" else (proxies[1], "SubpelConv2xProxy")
    with _refused(f"{cls}.{method}", named):
        getattr(proxy, method)(*make())
    assert rec.calls == []


@gpu
def test_a_proxy_without_parameters_is_refused(rec):
    from opendcvc_amd import ops
    from opendcvc_amd._lib import DcvcError
    with pytest.raises(DcvcError, match="set_param"):
        ops.DepthConvProxy().forward(T(1, 24, 2, 3))
    with pytest.raises(DcvcError, match="set_param"):
        ops.SubpelConv2xProxy().forward_with_cat(T(1, 16, 2, 3), T(1, 5, 4, 6), True)
    assert rec.calls == []
