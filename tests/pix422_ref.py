"""numpy restatement of 4:2:2 frame I/O, written from docs/pixel_formats_422.md (not from csrc/dcvc_pix422.hip): the layouts
(pack / unpack / row_bytes) and the arithmetic (load_ref / store_ref / metric_planes_ref), every fp32 operation on its own in
the stated order.  tests/test_pix422_host.py pins the layouts against literal bytes; tests/test_gpu_pix422.py compares the
kernels with it bit for bit.  A frame "as a file holds it" is a list: [y, u, v] (uint8 / uint16) for a planar format, [surface]
(uint8 [H, row_bytes]) for a packed one."""
import numpy as np

F = np.float32
# name: (packing, bits)
FORMATS = {"yuv422p": ("planar", 8), "yuv422p10le": ("planar", 10), "yuv422p12le": ("planar", 12), "yuv422p16le": ("planar", 16),
           "uyvy422": ("uyvy", 8), "yuyv422": ("yuyv", 8), "v210": ("v210", 10)}
LAYOUT = {"planar": 0, "uyvy": 1, "yuyv": 2, "v210": 3}
# positions of (Y0, Y1, U, V) among the four bytes of a macropixel
_BYTES = {"uyvy": (1, 3, 0, 2), "yuyv": (0, 2, 1, 3)}


def bits_of(fmt):
    return FORMATS[fmt][1]


def packing_of(fmt):
    return FORMATS[fmt][0]


def sample_dtype(bits):
    return np.dtype("<u2") if bits > 8 else np.dtype(np.uint8)


def row_bytes(fmt, w):
    """bytes of a row of the surface of a packed format (v210: whole 48-pixel blocks of 128 bytes); of a luma row otherwise"""
    packing, bits = FORMATS[fmt]
    assert w > 0 and w % 2 == 0
    if packing == "v210":
        return (w + 47) // 48 * 128
    return 2 * w if packing != "planar" else w * sample_dtype(bits).itemsize


def random_planes(rng, h, w, bits):
    """low-aligned planar 4:2:2 samples (y [h, w], u, v [h, w / 2]) with both ends of the range present"""
    dt, hi = sample_dtype(bits), (1 << bits) - 1
    planes = [rng.integers(0, hi + 1, s).astype(dt) for s in ((h, w), (h, w // 2), (h, w // 2))]
    planes[0][0, 0], planes[0][-1, -1], planes[1][0, -1], planes[2][-1, 0] = 0, hi, hi, 0
    return planes


def pack(planes, fmt):
    """low-aligned planar planes (y [h, w], u, v [h, w / 2]) -> the frame as a file holds it"""
    packing, bits = FORMATS[fmt]
    y, u, v = (np.asarray(p) for p in planes)
    h, w = y.shape
    assert u.shape == v.shape == (h, w // 2) and max(int(p.max()) for p in (y, u, v)) < 1 << bits
    if packing == "planar":
        return [p.astype(sample_dtype(bits)) for p in (y, u, v)]
    if packing in _BYTES:
        s = np.zeros((h, w // 2, 4), np.uint8)
        y0, y1, pu, pv = _BYTES[packing]
        s[:, :, y0], s[:, :, y1], s[:, :, pu], s[:, :, pv] = y[:, 0::2], y[:, 1::2], u, v
        return [s.reshape(h, 2 * w)]
    groups = (w + 5) // 6
    # pixels at or beyond w are written as zero, and so are the groups that fill the row up to a multiple of 128 bytes
    Y, Cb, Cr = (np.zeros((h, groups * n), np.uint32) for n in (6, 3, 3))
    Y[:, :w], Cb[:, :w // 2], Cr[:, :w // 2] = y, u, v
    Y, Cb, Cr = Y.reshape(h, groups, 6), Cb.reshape(h, groups, 3), Cr.reshape(h, groups, 3)
    words = np.zeros((h, row_bytes(fmt, w) // 4), np.uint32)
    g = words[:, :4 * groups].reshape(h, groups, 4)
    g[:, :, 0] = Cb[:, :, 0] | Y[:, :, 0] << 10 | Cr[:, :, 0] << 20
    g[:, :, 1] = Y[:, :, 1] | Cb[:, :, 1] << 10 | Y[:, :, 2] << 20
    g[:, :, 2] = Cr[:, :, 1] | Y[:, :, 3] << 10 | Cb[:, :, 2] << 20
    g[:, :, 3] = Y[:, :, 4] | Cr[:, :, 2] << 10 | Y[:, :, 5] << 20
    return [words.astype("<u4").view(np.uint8).reshape(h, -1)]


def unpack(frame, fmt, w):
    """the frame as a file holds it (a surface may be wider than its row: a pitch) -> low-aligned planar (y, u, v)"""
    packing, bits = FORMATS[fmt]
    if packing == "planar":
        return [np.asarray(p) for p in frame]
    s = np.ascontiguousarray(np.asarray(frame[0])[:, :row_bytes(fmt, w)])
    h = s.shape[0]
    if packing in _BYTES:
        m = s.reshape(h, w // 2, 4)
        y0, y1, pu, pv = _BYTES[packing]
        y = np.empty((h, w), np.uint8)
        y[:, 0::2], y[:, 1::2] = m[:, :, y0], m[:, :, y1]
        return [y, m[:, :, pu].copy(), m[:, :, pv].copy()]
    g = s.view("<u4").reshape(h, -1, 4).astype(np.uint32)
    lo, mid, hi = g & 1023, (g >> 10) & 1023, (g >> 20) & 1023
    Y = np.stack([mid[:, :, 0], lo[:, :, 1], hi[:, :, 1], mid[:, :, 2], lo[:, :, 3], hi[:, :, 3]], axis=2).reshape(h, -1)
    Cb = np.stack([lo[:, :, 0], mid[:, :, 1], hi[:, :, 2]], axis=2).reshape(h, -1)
    Cr = np.stack([hi[:, :, 0], lo[:, :, 2], mid[:, :, 3]], axis=2).reshape(h, -1)
    return [p.astype(np.uint16) for p in (Y[:, :w], Cb[:, :w // 2], Cr[:, :w // 2])]


def load_ref(frame, fmt, dtype, w=None, pad_to=16, pad=None):
    """the frame as a file holds it -> padded model input [1, 3, H', W']: sample / max_val as an fp32 division, ONE rounding
    to dtype, chroma columns doubled, replicate pad (to a multiple of pad_to, or by pad = (pad_b, pad_r))"""
    if w is None:
        assert packing_of(fmt) != "v210"
        w = frame[0].shape[1] // (1 if packing_of(fmt) == "planar" else 2)
    max_val = F((1 << bits_of(fmt)) - 1)
    y, u, v = ((p.astype(F) / max_val).astype(dtype) for p in unpack(frame, fmt, w))
    x = np.stack([y, np.repeat(u, 2, axis=1), np.repeat(v, 2, axis=1)])
    h = y.shape[0]
    pb, pr = pad if pad is not None else ((-h) % pad_to, (-w) % pad_to)
    return np.ascontiguousarray(np.pad(x, ((0, 0), (0, pb), (0, pr)), mode="edge")[None])


def metric_planes_ref(x, h, w, bits):
    """model frame [1, 3, H', W'] (fp16 / fp32) -> fp32 planes clip(., 0, 1) * max_val, y [h, w], u / v [h, w / 2] with the
    fp32 chroma (a + b) * 0.5 over the pixel pair; not rounded"""
    max_val = F((1 << bits) - 1)
    x = x[0, :, :h, :w].astype(F)
    c = ((x[1:, :, 0::2] + x[1:, :, 1::2]) * F(0.5)).astype(F)
    scale = lambda p: (np.clip(p, F(0), F(1)) * max_val).astype(F)
    return scale(x[0]), scale(c[0]), scale(c[1])


def store_planes_ref(x, h, w, bits):
    """-> low-aligned planar (y, u, v): the metric planes rounded to nearest even and clipped"""
    max_val = (1 << bits) - 1
    return [np.clip(np.rint(p), 0, max_val).astype(sample_dtype(bits)) for p in metric_planes_ref(x, h, w, bits)]


def store_ref(x, h, w, fmt):
    """-> the frame as a file holds it"""
    return pack(store_planes_ref(x, h, w, bits_of(fmt)), fmt)
