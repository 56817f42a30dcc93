"""4:2:2 frame I/O (csrc/dcvc_pix422.hip, docs/pixel_formats_422.md): what SDI capture cards and mezzanine files deliver -
planar yuv422p / yuv422p10le .., the packed 8-bit surfaces uyvy422 / yuyv422 and the packed 10-bit surface v210 - read into
and written from model frames on the device.  pipeline.PixelFormat keeps its own table (4:2:0 and 4:4:4); this module is
the 4:2:2 counterpart of its load_frame / store_frame and of harness.RawVideoReader.  A packed frame is ONE surface, a
[H, pitch] uint8 tensor whose rows hold row_bytes(width) bytes of samples."""
from dataclasses import dataclass

PLANAR, UYVY, YUYV, V210 = 0, 1, 2, 3            # DCVC_422_* of include/dcvc_amd.h
_PACKINGS = {"planar": PLANAR, "uyvy": UYVY, "yuyv": YUYV, "v210": V210}


@dataclass(frozen=True)
class Format422:
    """A 4:2:2 raw format: packing 'planar' (8 .. 16 bits, little-endian 16-bit words above 8, value in the low bits), 'uyvy' /
    'yuyv' (8 bits, bytes U Y0 V Y1 / Y0 U Y1 V per pixel pair) or 'v210' (10 bits, 6 pixels in four 32-bit words, rows
    padded to 128 bytes).  Format422.parse(name) knows the ffmpeg spellings of FORMATS_422."""
    name: str
    packing: str
    bit_depth: int
    chroma = 422

    def __post_init__(self):
        if self.packing not in _PACKINGS:
            raise ValueError(f"4:2:2 format {self.name!r}: packing {self.packing!r} (one of {', '.join(_PACKINGS)})")
        want = {"planar": range(8, 17), "uyvy": (8,), "yuyv": (8,), "v210": (10,)}[self.packing]
        if self.bit_depth not in want:
            raise ValueError(f"4:2:2 format {self.name!r}: {self.packing} with {self.bit_depth} bits")

    @staticmethod
    def parse(name):
        """'yuv422p10le', 'uyvy422', 'v210', ... -> Format422; ValueError for any other name"""
        if isinstance(name, Format422):
            return name
        try:
            return FORMATS_422[name]
        except (KeyError, TypeError):
            raise ValueError(f"unknown 4:2:2 format {name!r}: one of {', '.join(FORMATS_422)}") from None

    @property
    def layout(self):
        return _PACKINGS[self.packing]

    @property
    def packed(self):
        return self.packing != "planar"

    @property
    def max_val(self):
        return (1 << self.bit_depth) - 1

    @property
    def sample_bytes(self):
        """bytes of a planar sample (the samples of a packed surface are not byte-sized units: see row_bytes)"""
        return 2 if self.bit_depth > 8 else 1

    @property
    def numpy_dtype(self):
        import numpy as np
        return np.dtype("<u2") if self.bit_depth > 8 else np.dtype(np.uint8)

    @property
    def torch_dtype(self):
        import torch
        return torch.uint16 if self.bit_depth > 8 else torch.uint8

    def check_width(self, width):
        if width <= 0 or width % 2:
            raise ValueError(f"{self.name}: 4:2:2 needs a positive even width (got {width})")

    def row_bytes(self, width):
        """bytes of one row of a file: of the surface for a packed format (v210: whole 48-pixel blocks of 128 bytes), of the
        luma plane for a planar one"""
        self.check_width(width)
        if self.packing == "v210":
            return (width + 47) // 48 * 128
        return 2 * width if self.packed else width * self.sample_bytes

    def plane_shapes(self, height, width):
        """shapes of what a frame of a file holds, in file order: (y, u, v) in samples, or the one surface in bytes"""
        self.check_width(width)
        if self.packed:
            return ((height, self.row_bytes(width)),)
        return ((height, width), (height, width // 2), (height, width // 2))

    def frame_bytes(self, height, width):
        return height * self.row_bytes(width) * (1 if self.packed else 2)


FORMATS_422 = {f.name: f for f in (
    [Format422("yuv422p", "planar", 8)] + [Format422(f"yuv422p{b}le", "planar", b) for b in (10, 12, 16)] +
    [Format422("uyvy422", "uyvy", 8), Format422("yuyv422", "yuyv", 8), Format422("v210", "v210", 10)])}


def _as_list(planes_or_surface):
    import torch
    return [planes_or_surface] if isinstance(planes_or_surface, torch.Tensor) else list(planes_or_surface)


def load_frame_422(planes_or_surface, fmt, dtype, pad_to=16, height=None, width=None, strides=None):
    """device planes (y, u, v) or the surface of a Format422 -> padded model input [1,3,H',W'] (one kernel: sample / max_val
    as an fp32 division, one rounding to `dtype`, chroma columns doubled, replicate pad).  Planar: as pipeline.load_frame -
    tight [H, W] / [H, W/2] tensors, or strides=(y_stride, c_stride) in samples with height / width given.  Packed: a
    [H, pitch] uint8 tensor (or (surface,)); the pitch is the tensor's row length unless strides=(pitch_bytes, ..) says
    otherwise; width defaults to pitch / 2 for uyvy422 / yuyv422 and must be given for v210, whose rows are padded."""
    import torch
    from . import _lib
    from . import nn as L
    fmt = Format422.parse(fmt)
    planes = _as_list(planes_or_surface)
    if pad_to % 8:
        raise ValueError("pad_to must be a multiple of 8 (the kernels store 8 pixels at a time)")
    if len(planes) != (1 if fmt.packed else 3):
        raise ValueError(f"{fmt.name}: {1 if fmt.packed else 3} tensors expected, got {len(planes)}")
    if fmt.packed:
        s = planes[0]
        if s.element_size() != 1:
            raise ValueError(f"{fmt.name}: a uint8 surface is expected, got {s.dtype}")
        if strides is None:
            s = planes[0] = s.contiguous()
            if s.dim() != 2:
                raise ValueError(f"{fmt.name}: a [H, pitch] surface is expected, got {tuple(s.shape)}")
            height, pitch = s.shape
        else:
            pitch = strides[0] if isinstance(strides, (tuple, list)) else strides
        if width is None:
            if fmt.packing == "v210":
                raise ValueError("v210: the width must be given (a row is padded to whole 48-pixel blocks)")
            width = pitch // 2
        ptrs, ys, cs = [L._p(s), None, None], int(pitch), 0
    else:
        for p in planes:
            if p.element_size() != fmt.sample_bytes:
                raise ValueError(f"{fmt.name}: planes of {fmt.sample_bytes}-byte samples expected, got {p.dtype}")
        if strides is None:
            planes = [p.contiguous() for p in planes]
            height, width = planes[0].shape
            ys, cs = width, width // 2
        else:
            ys, cs = (int(s) for s in strides)
        ptrs = [L._p(p) for p in planes]
    fmt.check_width(width)
    pr, pb = (-width) % pad_to, (-height) % pad_to
    out = torch.empty((1, 3, height + pb, width + pr), dtype=dtype, device=planes[0].device)
    _lib.check(_lib.lib().dcvc_yuv422_to_frame(L.dtype_code(dtype), fmt.layout, fmt.bit_depth, *ptrs, ys, cs, height, width, pb, pr,
                                               L._p(out), L._stream()), "dcvc_yuv422_to_frame")
    return out


def store_frame_422(x_hat, height, width, fmt):
    """decoded [1,3,H',W'] -> what a file of the height x width picture holds in `fmt`: the device planes (y, u, v) (uint8 /
    torch.uint16) or (surface,), a tight [H, row_bytes(width)] uint8 tensor.  Crop, fp32, chroma (a + b) * 0.5 over the pixel
    pair, clip(., 0, 1) * max_val, round to nearest even, clip; every byte of a v210 row is written, filler zero."""
    import torch
    from . import _lib
    from . import nn as L
    fmt = Format422.parse(fmt)
    x = x_hat.contiguous()
    dt = torch.uint8 if fmt.packed else fmt.torch_dtype
    planes = [torch.empty(s, dtype=dt, device=x.device) for s in fmt.plane_shapes(height, width)]
    ptrs = [L._p(p) for p in planes] + [None] * (3 - len(planes))
    ys, cs = (fmt.row_bytes(width), 0) if fmt.packed else (width, width // 2)
    code, *frame = L.frame_args(x, (height, width))
    _lib.check(_lib.lib().dcvc_frame_to_yuv422(code, fmt.layout, fmt.bit_depth, *frame, *ptrs, ys, cs, L._stream()),
               "dcvc_frame_to_yuv422")
    return tuple(planes)


def unpack_422(planes_or_surface, fmt, width):
    """the planes of a Format422 source as the metrics read them: planar (y [H, W], u, v [H, W/2]), value in the low bits,
    uint8 or torch.uint16.  Planar formats pass through; a packed surface ([H, pitch] uint8) is taken apart with torch glue
    through int32 views: the measuring side, not the codec's path (as harness.source_planes does for NV12 / P010)."""
    import torch
    fmt = Format422.parse(fmt)
    planes = _as_list(planes_or_surface)
    if not fmt.packed:
        return planes
    if width is None:
        if fmt.packing == "v210":
            raise ValueError("v210: the width must be given (a row is padded to whole 48-pixel blocks)")
        width = planes[0].shape[1] // 2
    fmt.check_width(width)
    s = planes[0][:, :fmt.row_bytes(width)]
    if fmt.packing == "v210":
        w = s.contiguous().view(torch.int32)                                                     # [H, words]
        slots = torch.stack([w & 1023, (w >> 10) & 1023, (w >> 20) & 1023], dim=2).reshape(w.shape[0], -1)
        # slots of a group: Cb0 Y0 Cr0 Y1 Cb1 Y2 Cr1 Y3 Cb2 Y4 Cr2 Y5 - luma at the odd slots, Cb at 0 mod 4, Cr at 2 mod 4
        y, u, v = slots[:, 1::2][:, :width], slots[:, 0::4][:, :width // 2], slots[:, 2::4][:, :width // 2]
        return [p.to(torch.int16).contiguous().view(torch.uint16) for p in (y, u, v)]
    yo, uo, vo = (1, 0, 2) if fmt.packing == "uyvy" else (0, 1, 3)
    return [s[:, yo::2].contiguous(), s[:, uo::4].contiguous(), s[:, vo::4].contiguous()]


class Raw422Reader:
    """a raw file of a Format422: per frame (y, u, v), or (surface,) for a packed format, as numpy views of the frame's
    buffer - planes uint8 or little-endian uint16 as stored, a surface [H, row_bytes(width)] uint8 (a v210 file's rows have
    that length).  EOFError on a missing or short frame."""

    def __init__(self, path, width, height, fmt):
        self.fmt = Format422.parse(fmt)
        self.shapes = self.fmt.plane_shapes(height, width)
        self.frame_bytes = self.fmt.frame_bytes(height, width)
        self.f = open(path, "rb")

    def read(self):
        import numpy as np
        buf = self.f.read(self.frame_bytes)
        if len(buf) < self.frame_bytes:
            raise EOFError("raw video file ended")
        a = np.frombuffer(buf, np.uint8 if self.fmt.packed else self.fmt.numpy_dtype)
        planes, off = [], 0
        for h, w in self.shapes:
            planes.append(a[off:off + h * w].reshape(h, w))
            off += h * w
        return tuple(planes)

    def close(self):
        self.f.close()
