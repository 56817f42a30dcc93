"""numpy restatement of the frame I/O arithmetic of csrc/dcvc_pixfmt.hip (every fp32 operation on its own, in the stated
order), the second comparator of tests/test_gpu_pixfmt.py; tests/test_pixfmt_host.py pins it, on the CPU, against the
planes the reference family's reader / writer produced (tests/golden/frame_io_hbd.npz)."""
import numpy as np

F = np.float32
CASES = [(tag, chroma, bits) for tag in "abc" for chroma in (420, 444) for bits in (10, 12, 16)]


def sample_dtype(bits):
    return np.uint16 if bits > 8 else np.uint8


def split_planes(flat, h, w, chroma):
    """a frame in file order (y, u, v, flat) -> its three planes"""
    ch, cw = (h, w) if chroma == 444 else (h // 2, w // 2)
    assert flat.size == h * w + 2 * ch * cw
    return [flat[:h * w].reshape(h, w), flat[h * w:h * w + ch * cw].reshape(ch, cw), flat[h * w + ch * cw:].reshape(ch, cw)]


def fixture_size(gold, tag):
    return gold[f"rec_{tag}"].shape[1:]


def fixture_source(gold, tag, chroma, bits):
    """the b-bit source planes of a fixture case: the stored 16-bit planes shifted down to b bits (as the generator did)"""
    h, w = fixture_size(gold, tag)
    return split_planes((gold[f"src_{tag}_{chroma}"] >> (16 - bits)).astype(np.uint16), h, w, chroma)


def fixture_written(gold, tag, chroma, bits, name):
    """the planes the reference's writer wrote for the fp32 (name 'f32') / fp16 ('f16') reconstruction of the case"""
    h, w = fixture_size(gold, tag)
    return split_planes(gold[f"out_{tag}_{chroma}_{bits}_{name}"], h, w, chroma)


def fixture_reconstruction(gold, tag, dtype, pad_to=16):
    """the stored reconstruction [3, h, w] (fp32) as a padded model frame [1, 3, H', W'] of `dtype` (the values in the pad
    are never read by the store)"""
    x = gold[f"rec_{tag}"]
    _, h, w = x.shape
    x = np.pad(x, ((0, 0), (0, (-h) % pad_to), (0, (-w) % pad_to)), mode="edge")
    return np.ascontiguousarray(x[None].astype(dtype)), h, w


def load_ref(planes, chroma, bits, dtype, pad_to=16):
    """low-bit-aligned planar planes (y, u, v) -> padded model input [1, 3, H', W']: sample / max_val as an fp32 division,
    ONE rounding to dtype, nearest chroma up-sampling, replicate pad"""
    max_val = F((1 << bits) - 1)
    y, u, v = ((p.astype(F) / max_val).astype(dtype) for p in planes)
    if chroma == 420:
        u, v = (np.repeat(np.repeat(p, 2, axis=0), 2, axis=1) for p in (u, v))
    x = np.stack([y, u, v])
    h, w = y.shape
    return np.pad(x, ((0, 0), (0, (-h) % pad_to), (0, (-w) % pad_to)), mode="edge")[None]


def metric_planes_ref(x, h, w, chroma, bits):
    """model frame [1, 3, H', W'] (fp16 / fp32) -> fp32 planes clip(., 0, 1) * max_val, 4:2:0 chroma the fp32
    ((a + b) + (d + e)) * 0.25 over the 2x2 block; not rounded"""
    max_val = F((1 << bits) - 1)
    x = x[0, :, :h, :w].astype(F)
    y, c = x[0], x[1:]
    if chroma == 420:
        c = ((c[:, 0::2, 0::2] + c[:, 0::2, 1::2]) + (c[:, 1::2, 0::2] + c[:, 1::2, 1::2])) * F(0.25)
    scale = lambda p: (np.clip(p, F(0), F(1)) * max_val).astype(F)
    return scale(y), scale(c[0]), scale(c[1])


def store_ref(x, h, w, chroma, bits):
    """-> the low-bit-aligned planes (y, u, v) a file holds: the metric planes rounded to nearest even and clipped"""
    max_val = (1 << bits) - 1
    return tuple(np.clip(np.rint(p), 0, max_val).astype(sample_dtype(bits)) for p in metric_planes_ref(x, h, w, chroma, bits))


def interleave(u, v):
    """planar chroma -> the semi-planar plane [h, 2 w]: U, V, U, V, ..."""
    uv = np.empty((u.shape[0], 2 * u.shape[1]), u.dtype)
    uv[:, 0::2], uv[:, 1::2] = u, v
    return uv
