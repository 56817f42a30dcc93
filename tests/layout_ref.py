"""Plain numpy restatements of the layout kernels (csrc/dcvc_elem.hip) and the comparison helpers of the seam and layout
tests (tests/test_gpu_ops_seam.py, tests/test_gpu_layout.py).  The kernels move data, or multiply once in fp32 and round
once: every comparison here is on the bit patterns.  tests/test_layout_ref_host.py holds the restatements against
torch.nn.functional on the CPU and shows that each helper rejects a seeded mistake."""
import numpy as np

import layer_utils as LU


# ----------------------------------------------------------------------------- restatements (numpy, any dtype)

def nchw_to_hwc(x):
    """[1, C, H, W] -> [H, W, C]"""
    assert x.shape[0] == 1
    return np.ascontiguousarray(np.moveaxis(x[0], 0, 2))


def hwc_to_nchw(x):
    """[H, W, C] -> [1, C, H, W]"""
    return np.ascontiguousarray(np.moveaxis(x, 2, 0)[None])


def replicate_pad_hwc(x, pad_b, pad_r):
    """[H, W, C] -> [H + pad_b, W + pad_r, C]: the last row / column repeated"""
    H, W, _ = x.shape
    ys = np.minimum(np.arange(H + pad_b), H - 1)
    xs = np.minimum(np.arange(W + pad_r), W - 1)
    return np.ascontiguousarray(x[ys][:, xs])


def replicate_pad_nchw(x, pad_b, pad_r):
    """[B, C, H, W] -> [B, C, H + pad_b, W + pad_r]"""
    H, W = x.shape[2:]
    ys = np.minimum(np.arange(H + pad_b), H - 1)
    xs = np.minimum(np.arange(W + pad_r), W - 1)
    return np.ascontiguousarray(x[:, :, ys][:, :, :, xs])


def crop_hwc(x, H2, W2):
    return np.ascontiguousarray(x[:H2, :W2])


def unshuffle8(x):
    """PixelUnshuffle(8) of a [C, H, W] picture into HWC: [H / 8, W / 8, 64 C], channel c * 64 + dy * 8 + dx"""
    C, H, W = x.shape
    out = np.empty((H // 8, W // 8, C * 64), x.dtype)
    for c in range(C):
        for dy in range(8):
            for dx in range(8):
                out[:, :, c * 64 + dy * 8 + dx] = x[c, dy::8, dx::8]
    return out


def shuffle8(x):
    """PixelShuffle(8) of an HWC map [H, W, 64 C] into a [C, 8 H, 8 W] picture"""
    H, W, C64 = x.shape
    out = np.empty((C64 // 64, H * 8, W * 8), x.dtype)
    for c in range(C64 // 64):
        for dy in range(8):
            for dx in range(8):
                out[c, dy::8, dx::8] = x[:, :, c * 64 + dy * 8 + dx]
    return out


def shuffle8_nchw(x):
    """PixelShuffle(8) of [1, C, H, W] -> [1, C / 64, 8 H, 8 W]"""
    return shuffle8(nchw_to_hwc(x))[None]


def bias_clamp(x, bias, do_clamp):
    """dcvc_shuffle8_clamp / dcvc_op_bias_pixel_shuffle_8 before the move, per channel (last axis), in the order that
    tests/test_gpu_ops.py::test_unshuffle8_shuffle8_layout_kernels states: fp32 add, rounding to x's dtype, clamp (the
    kernels clamp in fp32 and round once: the same bits, a clamp to [0, 1] commutes with a monotonic rounding that keeps
    0 and 1)"""
    v = x.astype(np.float32)
    if bias is not None:
        v = (v + np.asarray(bias, np.float32)).astype(x.dtype).astype(np.float32)
    if do_clamp:
        v = np.clip(v, np.float32(0), np.float32(1))
    return v.astype(x.dtype)


def scale_channels(x, q):
    """(x.float() * q).to(dtype), q per channel (last axis)"""
    return (x.astype(np.float32) * np.asarray(q, np.float32)).astype(x.dtype)


# ----------------------------------------------------------------------------- comparison helpers

def to_np(t):
    """numpy array of a torch tensor (any device, any strides) or of an array-like"""
    if hasattr(t, "detach"):
        return t.detach().cpu().contiguous().numpy()
    return np.ascontiguousarray(t)


def bits(a):
    a = to_np(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def assert_same_bits(got, want, what):
    """shape, dtype and every bit pattern (so -0.0 != 0.0 and a NaN equals the same NaN)"""
    got, want = to_np(got), to_np(want)
    assert got.shape == want.shape, f"{what}: shape {got.shape}, expected {want.shape}"
    assert got.dtype == want.dtype, f"{what}: dtype {got.dtype}, expected {want.dtype}"
    bad = np.argwhere(bits(got) != bits(want))
    assert bad.shape[0] == 0, (f"{what}: {bad.shape[0]} of {got.size} elements differ, first at {bad[0].tolist()}: got "
                               f"{got[tuple(bad[0])]!r}, expected {want[tuple(bad[0])]!r}")


def assert_cat(result, out, to_cat, cat_at_front, what):
    """result == cat(to_cat, out) (front) or cat(out, to_cat) along the channels of NCHW, bit for bit, contiguous and of
    out's dtype"""
    assert result.is_contiguous(), f"{what}: the concatenation is not contiguous"
    assert result.dtype == out.dtype, f"{what}: {result.dtype}, expected {out.dtype}"
    parts = (to_np(to_cat), to_np(out)) if cat_at_front else (to_np(out), to_np(to_cat))
    assert_same_bits(result, np.concatenate(parts, axis=1), what)


def assert_pad_zero(x_hwc, C, what):
    """the channels from C on are zeros (+0.0: all bits clear)"""
    pad = bits(x_hwc)[..., C:]
    assert not pad.any(), f"{what}: {int(np.count_nonzero(pad))} pad channel entries are not zero"


# ----------------------------------------------------------------------------- operands inside 0xFF-filled buffers

def operand(values, shape, dtype, ld=None, off=0, band=64, device="cuda"):
    """(view, raw): a [..., C] view of `shape` whose leading axes are contiguous among themselves with row stride ld
    (default C) elements, inside the 1-D uint8 buffer `raw`, which is 0xFF everywhere else (and inside the view too when
    values is None: an output the kernel has to write).  Where the placement obeys layer_utils.guarded's 16-byte rule and
    the view is an [H, W, C] map, this IS layer_utils.guarded: the view starts (8 W + 16) * ld + off elements into `raw`
    (its guard band is counted in pixels; `band` is not used).  Otherwise the equivalent raw-buffer view (odd row strides,
    bases 2 / 4 / 8 bytes into the allocation, NCHW tensors), which starts band + off elements into `raw`, band rounded
    up to 16 bytes."""
    import torch
    es = LU._es(dtype)
    C = shape[-1]
    ld = C if ld is None else ld
    if len(shape) == 3 and (ld * es) % 16 == 0 and (off * es) % 16 == 0 and off + C <= ld:
        return LU.guarded(tuple(shape[:2]) if values is None else np.asarray(values), C, dtype, ld=ld, chan_off=off,
                          device=device)
    rows = int(np.prod(shape[:-1]))
    # the allocation is 256-byte aligned and band * es a multiple of 16: `off` alone decides the view's alignment
    band = (band * es + 15) // 16 * 16 // es
    raw = torch.full(((2 * band + off + rows * ld) * es,), 0xFF, dtype=torch.uint8, device=device)
    strides, s = [], ld
    for n in reversed(shape[:-1]):
        strides.insert(0, s)
        s *= n
    view = torch.as_strided(raw.view(dtype), tuple(shape), (*strides, 1), band + off)
    if values is not None:
        view.copy_(torch.as_tensor(np.array(values, copy=True)).to(dtype))
    return view, raw


def clean(raw, view):
    """True if every byte of `raw` outside `view` is still 0xFF (== layer_utils.untouched for a guarded view)"""
    import torch
    es = view.element_size()
    inside = torch.zeros(raw.numel() // es, dtype=torch.bool, device=raw.device)
    torch.as_strided(inside, view.shape, view.stride(), view.storage_offset()).fill_(True)
    changed = (raw.view(-1, es) != 0xFF).any(dim=1)
    return not bool((changed & ~inside).any())


def still_ff(t):
    """True if every byte of the tensor / view t is 0xFF (an output region the kernel must not write)"""
    import torch
    return t.numel() == 0 or bool((t.contiguous().view(torch.uint8) == 0xFF).all())
