"""numpy restatement of the element-per-thread frame I/O entries (dcvc_yuv420_to_frame, dcvc_frame_to_yuv420,
dcvc_rgb_to_frame, dcvc_frame_to_rgb of csrc/dcvc_pixfmt.hip, dcvc_frame_to_yuv420_planes of csrc/dcvc_metrics.hip): every
fp32 / fp16 operation on its own, in the order the kernel comments give.  An fp16 operation is restated as "compute in fp32,
round to fp16" (q below), which is what the kernels do.  tests/test_frame_io_ref_host.py pins it, on the CPU, to the fixtures
the reference harness's own functions produced (tests/golden/frame_io.npz, frame_io_rgb.npz); the GPU tests of
tests/test_gpu_frame_io_placement.py compare the kernels with it at the sizes and pads the fixtures do not have."""
import numpy as np

F = np.float32
KR, KG, KB = F(0.2126), F(0.7152), F(0.0722)          # BT.709, the fp32 values of the reference's Python floats


def q(v, dtype):
    """an fp32 value rounded to the storage type, back in fp32"""
    return v.astype(dtype).astype(F)


def edge_pad(x, pad_b, pad_r):
    """[3, h, w] -> [1, 3, h + pad_b, w + pad_r], the last row and column replicated"""
    return np.ascontiguousarray(np.pad(x, ((0, 0), (0, pad_b), (0, pad_r)), mode="edge")[None])


def yuv420_to_frame(y, u, v, dtype, pad_b, pad_r):
    """uint8 planes -> the padded 4:4:4 model input: /255 in fp32, ONE rounding, nearest chroma up-sampling, replicate pad
    (the pad of the up-sampled picture: the clamped luma coordinate halved, also where a pad is odd)"""
    y, u, v = ((p.astype(F) / F(255)).astype(dtype) for p in (y, u, v))
    u, v = (np.repeat(np.repeat(p, 2, axis=0), 2, axis=1) for p in (u, v))
    return edge_pad(np.stack([y, u, v]), pad_b, pad_r)


def yuv420_planes(x, h, w):
    """model frame [1, 3, Hp, Wp] -> clamp(. * 255, 0, 255) of luma and of the 2x2 chroma mean, in the storage type: the
    product rounded to the storage type, and so the mean (the four-term sum is formed in fp32, where it is exact for
    fp16 operands); only the h x w picture is read"""
    t = x.dtype
    p = x[0, :, :h, :w].astype(F)
    scale = lambda a: np.clip(q(a * F(255), t), F(0), F(255)).astype(t)
    c = p[1:]
    m = q(((c[:, 0::2, 0::2] + c[:, 0::2, 1::2]) + (c[:, 1::2, 0::2] + c[:, 1::2, 1::2])) * F(0.25), t)
    return scale(p[0]), scale(m[0]), scale(m[1])


def frame_to_yuv420(x, h, w, round_uv):
    """-> uint8 planes: luma rounded to nearest even, chroma truncated like `.to(uint8)` unless round_uv"""
    y, u, v = (p.astype(F) for p in yuv420_planes(x, h, w))
    c8 = (lambda p: np.rint(p).astype(np.uint8)) if round_uv else (lambda p: p.astype(np.uint8))
    return np.rint(y).astype(np.uint8), c8(u), c8(v)


def rgb_to_frame(rgb, dtype, pad_b, pad_r):
    """uint8 planar RGB [3, h, w] -> the padded YCbCr model input: /255, rgb2ycbcr in fp32 in the reference's operation
    order, clamp, ONE rounding to the storage type, replicate pad"""
    r, g, b = (rgb[k].astype(F) / F(255) for k in range(3))
    yy = (KR * r + KG * g) + KB * b
    cb = (F(0.5) * (b - yy)) / F(1.0 - 0.0722) + F(0.5)
    cr = (F(0.5) * (r - yy)) / F(1.0 - 0.2126) + F(0.5)
    return edge_pad(np.stack([np.clip(p, F(0), F(1)).astype(dtype) for p in (yy, cb, cr)]), pad_b, pad_r)


def frame_to_rgb(x, h, w):
    """model frame [1, 3, Hp, Wp] (YCbCr) -> clamp(ycbcr2rgb(x) * 255, 0, 255) of the h x w picture, [3, h, w] in the storage
    type: every operation rounded to the storage type (the scalars stay fp32)"""
    t = x.dtype
    yy, cb, cr = (x[0, k, :h, :w].astype(F) for k in range(3))
    sr, sb = F(2.0 - 2.0 * 0.2126), F(2.0 - 2.0 * 0.0722)
    r = q(yy + q(sr * q(cr - F(0.5), t), t), t)
    b = q(yy + q(sb * q(cb - F(0.5), t), t), t)
    g = q(q(q(yy - q(KR * r, t), t) - q(KB * b, t), t) / KG, t)
    out = lambda p: np.clip(q(np.clip(p, F(0), F(1)) * F(255), t), F(0), F(255)).astype(t)
    return np.stack([out(r), out(g), out(b)])
