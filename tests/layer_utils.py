"""Seeded layer weights shared by the GPU layer tests and the fp16 reference-fixture generator
(tests/golden/make_golden_f16.py): fixtures then only carry inputs and expected outputs - the weights are regenerated
from (seed, shape) on the GPU box."""
import numpy as np


def make_dcb_weights(rng, prefix, cin, c, adaptor):
    """state-dict entries of one DepthConvBlock (reference keys: layers.py:65-90), O(1) activations"""
    sd = {}

    def conv(name, co, ci, k=1, gain=1.0):
        sd[f"{prefix}.{name}.weight"] = (rng.standard_normal((co, ci, k, k)) * gain / np.sqrt(ci * k * k)).astype(np.float32)
        sd[f"{prefix}.{name}.bias"] = (rng.standard_normal(co) * 0.1).astype(np.float32)

    if adaptor:
        conv("adaptor", c, cin)
    conv("dc.0", c, c)
    sd[f"{prefix}.dc.2.weight"] = (rng.standard_normal((c, 1, 3, 3)) / 3).astype(np.float32)
    sd[f"{prefix}.dc.2.bias"] = (rng.standard_normal(c) * 0.1).astype(np.float32)
    conv("dc.3", c, c, gain=0.5)
    conv("ffn.0", 4 * c, c)
    conv("ffn.2", c, 2 * c, gain=0.5)
    return sd


# the block's parameters in the order DepthConvProxy.set_param takes them (set_param_with_adaptor: then the adaptor's two)
DCB_PROXY_PARAMS = ["dc.0.weight", "dc.0.bias", "dc.2.weight", "dc.2.bias", "dc.3.weight", "dc.3.bias", "ffn.0.weight",
                    "ffn.0.bias", "ffn.2.weight", "ffn.2.bias"]


def make_conv_weights(rng, prefix, cout, cin, k):
    return {f"{prefix}.weight": (rng.standard_normal((cout, cin, k, k)) / np.sqrt(cin * k * k)).astype(np.float32),
            f"{prefix}.bias": (rng.standard_normal(cout) * 0.1).astype(np.float32)}


# fp16 layer cases pinned against the REFERENCE's own .half() run (tests/golden/ops_small_f16.npz):
# name, cin, c, adaptor, shortcut, quant, H, W, seed
F16_DCB_CASES = [
    ("dcb256", 256, 256, False, False, False, 16, 24, 9001),
    ("dcb256_q", 256, 256, False, False, True, 13, 21, 9002),
    ("dcb256_ad512", 512, 256, True, False, False, 9, 17, 9003),
    ("dcb128_short", 128, 128, False, True, False, 5, 7, 9004),
    ("dcb368_q", 368, 368, False, False, True, 10, 11, 9005),
    ("dcb320_ad256", 256, 320, True, False, False, 8, 10, 9006),
    ("dcb384_ad512", 512, 384, True, False, False, 7, 8, 9007),
    ("dcb512", 512, 512, False, False, False, 5, 9, 9008),
    ("dcb256_large", 256, 256, False, True, True, 96, 130, 9009),       # 12 480 px: the 128-pixel-tile kernels
]
# name, kind, cin, cout (after the shuffle for subpel), k, H, W, seed
F16_CONV_CASES = [
    ("subpel1", "subpel", 128, 128, 1, 9, 15, 9101),
    ("subpel3", "subpel", 128, 256, 3, 8, 12, 9102),
    ("conv3s2", "s2", 256, 128, 3, 14, 22, 9103),
    ("conv2s2", "s2", 128, 128, 2, 12, 20, 9104),
    ("conv1x1", "plain", 384, 256, 1, 9, 13, 9105),
]
F16_LARGE_KEEP = 16        # channels of the large-map case kept in the fixture


def f16_dcb_inputs(case):
    """(state dict, x fp16 [1, cin, H, W], q fp32 [c] or None) of a F16_DCB_CASES entry - the same draw order in the
    generator (build container) and in the GPU test"""
    name, cin, c, adaptor, shortcut, quant, H, W, seed = case
    rng = np.random.default_rng(seed)
    sd = make_dcb_weights(rng, "m", cin, c, adaptor)
    x = rng.standard_normal((1, cin, H, W)).astype(np.float16)
    q = rng.uniform(0.5, 1.5, c).astype(np.float32) if quant else None
    return sd, x, q


def f16_conv_inputs(case):
    name, kind, cin, cout, k, H, W, seed = case
    rng = np.random.default_rng(seed)
    prefix = "m.conv.0" if kind == "subpel" else "m"
    sd = make_conv_weights(rng, prefix, cout * 4 if kind == "subpel" else cout, cin, k)
    x = rng.standard_normal((1, cin, H, W)).astype(np.float16)
    return sd, x


# ----------------------------------------------------------------------------- placement helpers
# The layer kernels take any channel-slice view of an HWC map whose base and row stride are 16-byte aligned, a scratch
# with arbitrary contents and float vectors of exactly the documented length.  These helpers build such operands inside
# NaN-filled buffers (every byte 0xFF: a NaN as fp16 and as fp32), so that a read outside an operand poisons the result and
# a write outside it changes a byte the test can see.  (tests/test_layer_placement_host.py checks them on the CPU.)

def _es(dtype):
    import torch
    return torch.empty((), dtype=dtype).element_size()


def guarded(values_hwc, c_phys, dtype, ld=None, chan_off=None, band=None, device="cuda"):
    """(view, raw): an [H, W, c_phys] view with strides (W * ld, ld, 1) inside the 1-D uint8 buffer `raw`, which is 0xFF
    everywhere else.  values_hwc: [H, W, C] numbers (C <= c_phys; the pad channels are zeros), or an (H, W) tuple: the
    view stays NaN too (an output the kernel has to write completely).  Defaults: row stride ld = c_phys + 32 elements,
    chan_off = 16 bytes' worth of elements (the contract's minimum alignment) in front of the channels, band = 8 W + 16
    guard pixels in front of and behind the map (the largest tile is 8 x 16: a ragged tile's full extent and a halo pixel
    at (-1, -1) or (H, W) still lie inside `raw`)."""
    import torch
    es = _es(dtype)
    if isinstance(values_hwc, tuple):
        (H, W), vals = values_hwc, None
    else:
        (H, W, C), vals = values_hwc.shape, values_hwc
        if C > c_phys:
            raise ValueError(f"{C} channels do not fit {c_phys} physical ones")
    ld = c_phys + 32 if ld is None else ld
    chan_off = 16 // es if chan_off is None else chan_off
    band = 8 * W + 16 if band is None else band
    if (ld * es) % 16 or (chan_off * es) % 16:
        raise ValueError(f"row stride {ld} / channel offset {chan_off} of {es}-byte elements break the 16-byte rule")
    if chan_off < 0 or band < 0 or chan_off + c_phys > ld:
        raise ValueError(f"channels {chan_off} .. {chan_off + c_phys} do not fit a row of {ld}")
    raw = torch.full(((2 * band + H * W) * ld * es,), 0xFF, dtype=torch.uint8, device=device)
    # = raw.view(dtype).view(-1, ld)[band:band + H * W, chan_off:chan_off + c_phys].unflatten(0, (H, W)), with these strides
    # on a map one pixel wide or high too (where torch is free to name others, and touched() could not find ld again)
    view = torch.as_strided(raw.view(dtype), (H, W, c_phys), (W * ld, ld, 1), band * ld + chan_off)
    if vals is not None:
        view.zero_()
        view[..., :C] = torch.as_tensor(np.array(vals, copy=True)).to(dtype).to(device)
    return view, raw


def touched(raw, view):
    """indices of the bytes of `raw` outside `view` that are no longer 0xFF"""
    import torch
    es, ld = view.element_size(), view.stride(1)
    H, W, cp = view.shape
    band, chan_off = divmod(view.storage_offset(), ld)
    outside = torch.ones(raw.numel(), dtype=torch.bool, device=raw.device)
    outside.view(-1, ld * es)[band:band + H * W, chan_off * es:(chan_off + cp) * es] = False
    return torch.nonzero(outside & (raw != 0xFF)).flatten()


def untouched(raw, view):
    return touched(raw, view).numel() == 0


def describe_touched(raw, view, limit=6):
    """the first touched bytes as (pixel relative to the map's first, element relative to the view's first channel)"""
    es, ld = view.element_size(), view.stride(1)
    band, chan_off = divmod(view.storage_offset(), ld)
    idx = touched(raw, view)
    where = [(int(i) // (ld * es) - band, int(i) % (ld * es) // es - chan_off) for i in idx[:limit]]
    return f"{idx.numel()} guard bytes written, first at (pixel, channel) {where}"


VEC_GUARD = 4      # floats of NaN in front of and behind a guarded vector (16 bytes: the vector stays 16-byte aligned)


def guarded_vec(values_f32, device="cuda"):
    """(vec, raw): exactly len(values_f32) floats with NaN on both sides"""
    import torch
    vals = torch.as_tensor(np.array(values_f32, dtype=np.float32, copy=True)).flatten()
    raw = torch.full(((2 * VEC_GUARD + vals.numel()) * 4,), 0xFF, dtype=torch.uint8, device=device)
    vec = raw.view(torch.float32)[VEC_GUARD:VEC_GUARD + vals.numel()]
    vec.copy_(vals)
    return vec, raw


def poison_scratch(nbytes, device="cuda"):
    """the layers' scratch of at least nbytes, every byte of it 0xFF: what a launch reads there without having written it
    in this run is a NaN, not the previous run's value"""
    import torch
    from opendcvc_amd import nn
    device = torch.empty(0, device=device).device      # with its index, as the layers name it (the pool's key)
    return nn.Scratch.get(nbytes, device).fill_(0xFF)


class GuardedRun:
    """The operands of one guarded run and what must hold of them afterwards.  src / vec / out hand out guarded operands
    (the second source with another row stride and channel offset than the first); check(): every output is finite, its
    pad channels are zeros, no byte around it has changed, and every source and vector buffer is byte-identical to its
    copy from before the call."""

    def __init__(self, dtype, device="cuda"):
        self.dtype, self.device = dtype, device
        self.inputs, self.outputs = [], []

    def _keep(self, name, raw):
        self.inputs.append((name, raw, raw.clone()))

    def src(self, values_hwc, c_phys, second=False):
        kw = dict(ld=c_phys + 64, chan_off=3 * (16 // _es(self.dtype))) if second else {}
        view, raw = guarded(values_hwc, c_phys, self.dtype, device=self.device, **kw)
        self._keep("x1" if second else "x0", raw)
        return view

    def vec(self, values_f32, name="vector"):
        if values_f32 is None:
            return None
        vec, raw = guarded_vec(values_f32, self.device)
        self._keep(name, raw)
        return vec

    def out(self, H, W, c_phys, c_log=None, ld=None, chan_off=None):
        view, raw = guarded((H, W), c_phys, self.dtype, ld=c_phys + 96 if ld is None else ld, chan_off=chan_off,
                            device=self.device)
        self.outputs.append((view, raw, c_phys if c_log is None else c_log))
        return view

    def scratch(self, nbytes):
        return poison_scratch(nbytes, self.device)

    def check(self):
        import torch
        if self.device != "cpu":
            torch.cuda.synchronize()
        for view, raw, c_log in self.outputs:
            bad = torch.nonzero(~torch.isfinite(view))
            assert bad.numel() == 0, f"{bad.shape[0]} non-finite output values, first at (y, x, c) {bad[:6].tolist()}"
            assert not bool(view[..., c_log:].any()), "pad channels must stay zero"
            assert untouched(raw, view), "output: " + describe_touched(raw, view)
        for name, raw, before in self.inputs:
            assert torch.equal(raw, before), f"{name}: the call changed its input buffer"
