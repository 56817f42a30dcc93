"""One rate point (or a qp sweep) over one planar 8-bit YUV 4:2:0 sequence on the HIP path, logged in the
reference's JSON schema - SURVEY.md section 8(f)-3.

Restates (no code shared) the behaviour of the reference harness:
  test_video.py:130-353   run_one_point_with_stream: encode every frame into the NAL container, write the
                          .bin, decode it back, distortion per decoded frame, timing, JSON log
  test_video.py:94-127    get_distortion (YUV 4:2:0: per-plane PSNR, combined (6 Y + U + V) / 8)
  test_video.py:448-463   the qp points of a sweep
  src/utils/metrics.py:81-96   calc_psnr
  src/utils/common.py:63-177   generate_log_json
  test_video.py:381-442,472-532   the job fan-out: a JSON dataset manifest, one job per (sequence, rate point), a pool
                          of spawned worker processes (-w), worker n on GPU n % gpu_num, one merged JSON log
  src/utils/common.py:49-60      dump_json (floats with six digits)
  test_video.py:66-127, src/utils/video_reader.py:10-47, transforms.py:27-53, metrics.py:9-79   PNG (RGB) sources: BT.709
                          rgb <-> ycbcr around the codec, RGB PSNR; --calc_ssim: MS-SSIM per plane (YUV: (6 Y + U + V) / 8)
Beyond the reference's two source types: raw files of the other pixel formats (pipeline.PIXEL_FORMATS: 10 / 12 / 16 bits,
4:4:4, NV12, P010) with the reference family's reader / writer arithmetic (DCVC-FM src/utils/video_reader.py:130-181,
video_writer.py:85-128) - RawVideoReader, pixfmt_distortion, the frame I/O kernels of csrc/dcvc_pixfmt.hip.
The codec calls are the drop-in DMCI / DMC of opendcvc_amd.models.

    python -m opendcvc_amd.harness --test-config cfg.json -w 16 --gpus 8 --output-path out.json     # configs[4]
"""
import importlib
import io
import json
import math
import os
import time

import numpy as np

from .bitstream import StreamWriter
from .pipeline import (PIXEL_FORMATS, PixelFormat, SequenceEncoder, StreamDecoder, load_frame, load_yuv420_frame, store_frame,
                       store_yuv420_frame, use_two_entropy_coders)
from .pix422 import FORMATS_422
from .repeat import tol_fraction

SRC_TYPES = ("yuv420", "png") + tuple(PIXEL_FORMATS)     # "yuv420": planar 8-bit 4:2:0 with the reference harness's arithmetic
SRC_TYPES_422 = tuple(FORMATS_422)                       # the 4:2:2 formats (pix422.py): planar, uyvy422, yuyv422, v210


# ---------------------------------------------------------------------------------- metrics / log
def psnr_from_mse(mse, data_range=255.0):
    """metrics.py:81-96: -999.9 for nan/inf, 999.9 below 1e-10, capped at 99.9"""
    if math.isnan(mse) or math.isinf(mse):
        return -999.9
    psnr = 10.0 * math.log10(data_range * data_range / mse) if mse > 1e-10 else 999.9
    return min(psnr, 99.9)


def calc_psnr(a, b, data_range=255.0):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return psnr_from_mse(float(np.mean(np.square(a - b))), data_range)


def _yuv420_metric_planes(x_hat, H, W):
    """the planes the host metrics of a YUV 4:2:0 source compare: the H x W crop of x_hat [1,3,H',W'], clamped, NOT rounded
    (chroma = 2x2 mean), in the reconstruction's own dtype like the reference's tensors -> (y, u, v)"""
    import torch
    x = x_hat[:, :, :H, :W]
    y_rec = torch.clamp(x[:, :1] * 255, 0, 255)
    uv_rec = torch.clamp(torch.nn.functional.avg_pool2d(x[:, 1:], 2) * 255, 0, 255)
    return y_rec[0, 0], uv_rec[0, 0], uv_rec[0, 1]


def yuv420_distortion(x_hat, y, u, v):
    """test_video.py:94-111 on the device: x_hat [1,3,H',W'] (model dtype, cropped here), y/u/v uint8 planes.
    PSNR of the planes of _yuv420_metric_planes; squared errors are summed in float64."""
    import torch
    out = [psnr_from_mse(float(torch.mean(torch.square(rec.double() - src.double()))))
           for rec, src in zip(_yuv420_metric_planes(x_hat, *y.shape), (y, u, v))]
    return [(6 * out[0] + out[1] + out[2]) / 8] + out


# MS-SSIM as the reference computes it for --calc_ssim (metrics.py:9-79: the multi-scale SSIM of Wang et al. with an 11x11 Gaussian
# window, sigma 1.5, 'valid' windows, 2x2 box + decimation between the scales, four scales instead of five below 176 pixels -
# "according to HM" - and none below 88).  Host numpy / scipy, like the reference's: a metric of the harness, not the hot path.
_MSSSIM_WEIGHTS = {5: (0.0448, 0.2856, 0.3001, 0.2363, 0.1333), 4: (0.0517, 0.3295, 0.3462, 0.2726)}


def _gauss_window(size=11, sigma=1.5):
    ax = np.arange(size, dtype=np.float64) - size // 2
    g = np.exp(-(ax[:, None] ** 2 + ax[None, :] ** 2) / (2.0 * sigma * sigma))
    return g / g.sum()


def _ssim_and_cs(a, b, window, data_range):
    from scipy import signal
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    local = lambda img: signal.fftconvolve(window, img, mode="valid")
    mu_a, mu_b = local(a), local(b)
    var_a, var_b, cov = local(a * a) - mu_a * mu_a, local(b * b) - mu_b * mu_b, local(a * b) - mu_a * mu_b
    cs = (2.0 * cov + c2) / (var_a + var_b + c2)
    return ((2 * mu_a * mu_b + c1) * (2 * cov + c2)) / ((mu_a * mu_a + mu_b * mu_b + c1) * (var_a + var_b + c2)), cs


def calc_msssim(a, b, data_range=255):
    """a, b: 2-D arrays (one plane each)"""
    from scipy import ndimage
    h, w = a.shape
    if h < 88 or w < 88:
        raise ValueError("MS-SSIM needs planes of at least 88 x 88 (the reference asserts)")
    levels = 5 if (h >= 176 and w >= 176) else 4
    weights = np.asarray(_MSSSIM_WEIGHTS[levels])
    window, box = _gauss_window(), np.full((2, 2), 0.25)
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    ssim_mean, cs_mean = [], []
    for _ in range(levels):
        ssim_map, cs_map = _ssim_and_cs(a, b, window, data_range)
        ssim_mean.append(ssim_map.mean())
        cs_mean.append(cs_map.mean())
        a = ndimage.convolve(a, box, mode="reflect")[::2, ::2]
        b = ndimage.convolve(b, box, mode="reflect")[::2, ::2]
    cs_mean, ssim_mean = np.asarray(cs_mean), np.asarray(ssim_mean)
    with np.errstate(invalid="ignore"):       # (unrelated pictures: a negative contrast term to a fractional power is NaN, as in the reference)
        return float(np.prod(cs_mean[:levels - 1] ** weights[:levels - 1]) * ssim_mean[levels - 1] ** weights[levels - 1])


def calc_msssim_rgb(a, b, data_range=255):
    """a, b: [3, H, W]; the mean over the three planes"""
    return sum(calc_msssim(a[i], b[i], data_range) for i in range(3)) / 3


def rgb_distortion(x_hat, rgb, calc_ssim=False):
    """test_video.py:116-126 on the device: x_hat [1,3,H',W'] YCbCr (model dtype), rgb uint8 [3,H,W] (device) ->
    ([psnr], [msssim]): clamp(ycbcr2rgb(x_hat) * 255, 0, 255) in the reconstruction's own dtype (one fused kernel), squared
    errors in float64; MS-SSIM on the host."""
    import torch
    rec = reconstruct_rgb(x_hat, rgb.shape[1], rgb.shape[2])
    psnr = psnr_from_mse(float(torch.mean(torch.square(rec.double() - rgb.double()))))
    ms = calc_msssim_rgb(rgb.cpu().numpy(), rec.float().cpu().numpy().astype(np.float64)) if calc_ssim else 0.0
    return [psnr], [ms]


def reconstruct_rgb(x_hat, height, width):
    """decoded [1,3,H',W'] YCbCr -> clamp(ycbcr2rgb * 255, 0, 255) of the height x width picture, [3,H,W] in x_hat's dtype
    (transforms.py:41-53, test_video.py:118-119)"""
    import torch
    from . import _lib
    from . import nn as L
    x = x_hat.contiguous()
    out = torch.empty((3, height, width), dtype=x.dtype, device=x.device)
    _lib.check(_lib.lib().dcvc_frame_to_rgb(*L.frame_args(x, (height, width)), L._p(out), L._stream()), "dcvc_frame_to_rgb")
    return out


def load_rgb_frame(rgb, dtype, pad_to=16):
    """uint8 device tensor [3,H,W] (RGB) -> padded YCbCr model input [1,3,H',W'] (one fused kernel; reference:
    np_image_to_tensor + rgb2ycbcr + the cast + replicate_pad, test_video.py:59-63,84-90,179)"""
    import torch
    from . import _lib
    from . import nn as L
    _, H, W = rgb.shape
    pr, pb = (-W) % pad_to, (-H) % pad_to
    out = torch.empty((1, 3, H + pb, W + pr), dtype=dtype, device=rgb.device)
    _lib.check(_lib.lib().dcvc_rgb_to_frame(L.dtype_code(dtype), L._p(rgb.contiguous()), H, W, pb, pr, L._p(out),
                                            L._stream()), "dcvc_rgb_to_frame")
    return out


def yuv420_msssim(x_hat, y, u, v):
    """--calc_ssim on a YUV 4:2:0 source (test_video.py:106-112): MS-SSIM of the planes yuv420_distortion compares, combined
    (6 Y + U + V) / 8; host computation on the clamped, not rounded, planes"""
    vals = [calc_msssim(src.cpu().numpy(), rec.float().cpu().numpy().astype(np.float64))
            for rec, src in zip(_yuv420_metric_planes(x_hat, *y.shape), (y, u, v))]
    return [(6 * vals[0] + vals[1] + vals[2]) / 8] + vals


def source_planes(planes, fmt, width=None):
    """the planes of a PixelFormat or Format422 source as the metrics read them: planar (y, u, v), value in the LOW bits
    (width: the picture's, which a v210 surface does not tell; by default what a tight surface holds).  Planar
    low-aligned formats pass through; the chroma of a semi-planar source is de-interleaved and msb-aligned words are
    shifted down (torch glue through int16 / int32 views: the measuring side, not the codec's path)"""
    import torch
    if fmt.chroma == 422:                      # a pix422.Format422: a packed surface is taken apart, the width is the picture's
        from .pix422 import unpack_422
        return unpack_422(planes, fmt, width)
    planes = list(planes)
    if fmt.semi_planar:
        uv = planes[1].view(torch.int16) if fmt.sample_bytes == 2 else planes[1]
        planes = [planes[0]] + [uv[:, k::2].contiguous().view(planes[1].dtype) for k in (0, 1)]
    if fmt.msb_aligned and fmt.bit_depth < 16:
        shift = 16 - fmt.bit_depth
        planes = [((p.view(torch.int16).to(torch.int32) & 0xFFFF) >> shift).to(torch.int16).view(torch.uint16) for p in planes]
    return planes


def pixfmt_metric_planes(x_hat, height, width, fmt):
    """the planes the metrics of a PixelFormat / Format422 source compare, in torch: crop, fp32, 4:2:0 chroma the explicit fp32
    ((a + b) + (d + e)) * 0.25 over the 2x2 block, 4:2:2 chroma (a + b) * 0.5 over the pixel pair, clip(., 0, 1) * max_val,
    NOT rounded -> fp32 (y, u, v)"""
    import torch
    x = x_hat[0, :, :height, :width].float()
    y, c = x[0], x[1:]
    if fmt.chroma == 420:
        c = ((c[:, 0::2, 0::2] + c[:, 0::2, 1::2]) + (c[:, 1::2, 0::2] + c[:, 1::2, 1::2])) * 0.25
    elif fmt.chroma == 422:
        c = (c[:, :, 0::2] + c[:, :, 1::2]) * 0.5
    scale = lambda p: torch.clamp(p, 0.0, 1.0) * float(fmt.max_val)
    return scale(y), scale(c[0]), scale(c[1])


def pixfmt_distortion(x_hat, planes, fmt, calc_ssim=False, width=None):
    """host-path metrics of a PixelFormat source (the reference family's writer arithmetic before its rounding, PSNR and
    MS-SSIM with data_range = max_val): -> (psnr, msssim), each [(6 Y + U + V) / 8, Y, U, V]; squared errors and MS-SSIM
    in float64 on the host"""
    src = [p.cpu().numpy().astype(np.float64) for p in source_planes(planes, fmt, width)]
    H, W = src[0].shape
    rec = [p.cpu().numpy().astype(np.float64) for p in pixfmt_metric_planes(x_hat, H, W, fmt)]
    dr = float(fmt.max_val)
    psnr = [calc_psnr(s, r, dr) for s, r in zip(src, rec)]
    ms = [calc_msssim(s, r, dr) for s, r in zip(src, rec)] if calc_ssim else [0.0, 0.0, 0.0]
    comb = lambda m: [(6 * m[0] + m[1] + m[2]) / 8] + m
    return comb(psnr), comb(ms)


def summarize(frame_pixel_num, test_time, frame_types, bits, psnrs, ssims, verbose=False,
              avg_encoding_time=None, avg_decoding_time=None):
    """The reference's per-sequence log (common.py:63-177): averages over I frames (type 0), P frames and
    all frames of bpp / PSNR / MS-SSIM (plus the Y, U, V components when 4-tuples are given), optional
    per-frame lists, timings.  Same keys, same insertion order."""
    n = len(frame_types)
    P = np.asarray(psnrs, np.float64).reshape(n, -1)
    S = np.asarray(ssims, np.float64).reshape(n, -1)
    B = np.asarray(bits, np.float64)
    T = np.asarray(frame_types)
    yuv = P.shape[1] > 1
    if yuv and not (P.shape[1] == 4 and S.shape[1] == 4):
        raise ValueError("per-frame metrics must be 1 value or (all, y, u, v)")
    comp = (("", 0), ("_y", 1), ("_u", 2), ("_v", 3)) if yuv else (("", 0),)
    is_i = T == 0
    log = {"frame_pixel_num": frame_pixel_num, "i_frame_num": int(is_i.sum()), "p_frame_num": int((~is_i).sum())}

    def block(tag, sel, count):
        log[f"ave_{tag}_frame_bpp"] = float(B[sel].sum() / count / frame_pixel_num) if count else 0
        for kind, M in (("psnr", P), ("msssim", S)):
            log[f"ave_{tag}_frame_{kind}"] = float(M[sel, 0].sum() / count) if count else 0
        for kind, M in (("psnr", P), ("msssim", S)):
            for suffix, k in comp[1:]:
                log[f"ave_{tag}_frame_{kind}{suffix}"] = float(M[sel, k].sum() / count) if count else 0

    if log["i_frame_num"] == 0:
        raise ZeroDivisionError("a sequence log needs at least one I frame")
    block("i", is_i, log["i_frame_num"])
    if verbose:
        log["frame_bpp"] = list(B / frame_pixel_num)
        log["frame_psnr"] = [float(v) for v in P[:, 0]]
        log["frame_msssim"] = [float(v) for v in S[:, 0]]
        log["frame_type"] = list(frame_types)
        for kind, M in (("psnr", P), ("msssim", S)):
            for suffix, k in comp[1:]:
                log[f"frame_{kind}{suffix}"] = [float(v) for v in M[:, k]]
    log["test_time"] = test_time
    block("p", ~is_i, log["p_frame_num"])
    log["ave_all_frame_bpp"] = float(B.sum() / (n * frame_pixel_num))
    log["ave_all_frame_psnr"] = float(P[:, 0].sum() / n)
    log["ave_all_frame_msssim"] = float(S[:, 0].sum() / n)
    if avg_encoding_time is not None and avg_decoding_time is not None:
        log["avg_frame_encoding_time"] = avg_encoding_time
        log["avg_frame_decoding_time"] = avg_decoding_time
    for kind, M in (("psnr", P), ("msssim", S)):
        for suffix, k in comp[1:]:
            log[f"ave_all_frame_{kind}{suffix}"] = float(M[:, k].sum() / n)
    return log


def sweep_qps(rate_num, qp_num=64):
    """test_video.py:452-455: rate_num points spread over the qp range, rounded half up"""
    if not 2 <= rate_num <= qp_num:
        raise ValueError("rate_num must be in [2, qp_num]")
    return [int(i + 0.5) for i in np.linspace(0, qp_num - 1, num=rate_num)]


# ---------------------------------------------------------------------------------- sequence I/O
class YUV420FileReader:
    """planar 8-bit 4:2:0 (video_reader.py:50-90): Y (H x W), U, V (H/2 x W/2) per frame"""

    def __init__(self, path, width, height):
        self.f = open(path, "rb")
        self.w, self.h = width, height

    def read(self):
        ys, cs = self.w * self.h, (self.w // 2) * (self.h // 2)
        buf = self.f.read(ys + 2 * cs)
        if len(buf) < ys + 2 * cs:
            raise EOFError("YUV file ended")
        a = np.frombuffer(buf, np.uint8)
        return (a[:ys].reshape(self.h, self.w), a[ys:ys + cs].reshape(self.h // 2, self.w // 2),
                a[ys + cs:].reshape(self.h // 2, self.w // 2))

    def close(self):
        self.f.close()


class RawVideoReader:
    """a raw file of any PixelFormat: per frame its planes in file order as numpy views of the frame's buffer - (y, u, v),
    or (y, uv) for semi-planar (the interleaved plane stays interleaved), uint8 or little-endian uint16 as stored
    (msb-aligned words are not shifted: the loader does that).  EOFError on a missing or short frame."""

    def __init__(self, path, width, height, fmt):
        self.fmt = PixelFormat.parse(fmt)
        self.shapes = self.fmt.plane_shapes(height, width)
        self.frame_bytes = self.fmt.frame_bytes(height, width)
        self.f = open(path, "rb")

    def read(self):
        buf = self.f.read(self.frame_bytes)
        if len(buf) < self.frame_bytes:
            raise EOFError("raw video file ended")
        a = np.frombuffer(buf, self.fmt.numpy_dtype)
        planes, off = [], 0
        for h, w in self.shapes:
            planes.append(a[off:off + h * w].reshape(h, w))
            off += h * w
        return tuple(planes)

    def close(self):
        self.f.close()


class PNGSequenceReader:
    """a directory of im1.png, im2.png, ... or im00001.png, ... (video_reader.py:10-47): uint8 [3, H, W] RGB per frame"""

    def __init__(self, path, width, height, start_num=1):
        names = set(os.listdir(path))
        if "im1.png" in names:
            self.digits = 1
        elif "im00001.png" in names:
            self.digits = 5
        else:
            raise ValueError(f"{path}: unknown image naming convention (expected im1.png ... or im00001.png ...)")
        self.path, self.w, self.h, self.index = path, width, height, start_num

    def read(self):
        from PIL import Image
        name = os.path.join(self.path, "im%s.png" % str(self.index).zfill(self.digits))
        if not os.path.exists(name):
            raise EOFError("PNG sequence ended")
        rgb = np.asarray(Image.open(name).convert("RGB"), np.uint8).transpose(2, 0, 1)
        if rgb.shape != (3, self.h, self.w):
            raise ValueError(f"{name}: {rgb.shape[2]}x{rgb.shape[1]}, expected {self.w}x{self.h}")
        self.index += 1
        return (rgb,)

    def close(self):
        pass


def _to_device(planes, device):
    import torch
    return [torch.from_numpy(np.array(p, copy=True)).to(device) for p in planes]     # (the planes may be read-only views of the file buffer)


# ---------------------------------------------------------------------------------- the three source families
class _Source:
    """One source family as run_one_point needs it, put together by make_source: reader(), to_input(planes, dtype) -> the padded
    model input, distortion(x_hat, planes, calc_ssim, dm) -> (psnr, ssim) of one frame as summarize() takes them (dm: a
    metrics.DeviceMetrics, None: the host path) and the reconstruction writer - open_rec / write_rec / close_rec put the
    planes of stored_planes(shown) into one raw file.  chroma_lines: the rows of the model frame one chroma line of the source
    covers (2 where the loader doubles the rows of a 4:2:0 source, else 1).  stored(x) -> the planes a file of the picture x
    would hold, as reader() + _to_device hand them on and distortion() takes them (docs/deinterlace.md: the reference picture
    of a deinterlacing run)."""
    rec = None

    def __init__(self, width, height, make_reader, to_input, distortion, stored_planes=None, chroma_lines=1):
        self.w, self.h, self.make_reader, self.to_input = width, height, make_reader, to_input
        self.distortion, self.stored_planes, self.chroma_lines = distortion, stored_planes, chroma_lines

    def stored(self, x):
        return list(self.stored_planes(x))

    def reader(self):
        self.last_reader = self.make_reader()
        return self.last_reader

    def open_rec(self, rec_path):
        self.rec = open(rec_path, "wb") if rec_path else None

    def write_rec(self, shown, fi):
        if self.rec is not None:
            for plane in self.stored_planes(shown):
                self.rec.write(plane.cpu().numpy().tobytes())

    def close_rec(self):
        if self.rec is not None:
            self.rec.close()


class _PNGSource(_Source):      # the reconstruction: PNGs named like the source's, clamp * 255 rounded to uint8 (test_video.py:314-318)
    def stored(self, x):
        import torch
        return [reconstruct_rgb(x, self.h, self.w).float().round().to(torch.uint8)]

    def open_rec(self, rec_path):
        self.rec_dir = rec_path
        if rec_path:
            os.makedirs(rec_path, exist_ok=True)

    def write_rec(self, shown, fi):
        if self.rec_dir:
            from PIL import Image
            rgb8 = self.stored(shown)[0].cpu().numpy()
            name = "im%s.png" % str(fi + 1).zfill(self.last_reader.digits)
            Image.fromarray(rgb8.transpose(1, 2, 0)).save(os.path.join(self.rec_dir, name))


def make_source(src_type, path, width, height):
    """the source object of a src_type (SRC_TYPES, SRC_TYPES_422); touches no file.  The host metrics are looked up in this module when
    they are called."""
    if src_type in FORMATS_422:
        from .pix422 import Raw422Reader, load_frame_422, store_frame_422
        f422 = FORMATS_422[src_type]
        f422.check_width(width)                # (an odd width is refused here)
        # every chroma line is one row high; a packed frame travels as its one surface, whose width the picture's is
        return _Source(width, height, lambda: Raw422Reader(path, width, height, f422),
                       lambda p, dt: load_frame_422(p, f422, dt, width=width),
                       lambda x, p, ssim, dm: (dm.yuv(x, p, f422, ssim, width) if dm else pixfmt_distortion(x, p, f422, ssim, width)),
                       lambda shown: store_frame_422(shown, height, width, f422), 1)
    fmt = PIXEL_FORMATS.get(src_type)          # None: the reference harness's own two source types
    if fmt is not None:
        fmt.plane_shapes(height, width)        # (4:2:0 with an odd size is refused here)
        return _Source(width, height, lambda: RawVideoReader(path, width, height, fmt), lambda p, dt: load_frame(p, fmt, dt),
                       lambda x, p, ssim, dm: dm.yuv(x, p, fmt, ssim) if dm else pixfmt_distortion(x, p, fmt, ssim),
                       lambda shown: store_frame(shown, height, width, fmt),           # the source's own format
                       2 if fmt.chroma == 420 else 1)
    if src_type == "png":
        # (the PNG reader's planes are a transposed view: the kernels read them planar, as load_rgb_frame does)
        return _PNGSource(width, height, lambda: PNGSequenceReader(path, width, height), lambda p, dt: load_rgb_frame(p[0], dt),
                          lambda x, p, ssim, dm: dm.rgb(x, p[0].contiguous(), ssim) if dm else rgb_distortion(x, p[0], ssim))
    # planar 8-bit 4:2:0, the reference's arithmetic: stored with Y rounded and chroma truncated (test_video.py:307-311)
    def distortion(x, p, ssim, dm):
        if dm:
            return dm.yuv420(x, *p, ssim)
        return yuv420_distortion(x, *p), (yuv420_msssim(x, *p) if ssim else [0.0, 0.0, 0.0, 0.0])
    return _Source(width, height, lambda: YUV420FileReader(path, width, height), lambda p, dt: load_yuv420_frame(*p, dt),
                   distortion, lambda shown: store_yuv420_frame(shown, height, width), 2)


# ---------------------------------------------------------------------------------- one rate point
def parse_crop(text):
    """--crop: 'auto', or T:B:L:R[:Y:U:V] - the rows / columns to leave out at the top, bottom, left and right and the bars'
    colour in 8-bit codes (default 16:128:128) -> 'auto' or (top, bottom, left, right, (y, u, v))"""
    if text == "auto":
        return text
    parts = str(text).split(":")
    if len(parts) not in (4, 7) or not all(p.isdigit() for p in parts):
        raise ValueError(f"crop {text!r}: auto or TOP:BOTTOM:LEFT:RIGHT[:Y:U:V], e.g. 138:138:0:0")
    vals = [int(p) for p in parts]
    colour = tuple(vals[4:]) if len(vals) == 7 else (16, 128, 128)
    if any(v % 2 for v in vals[:4]) or any(c > 255 for c in colour):
        raise ValueError(f"crop {text!r}: even extents (4:2:0 chroma) and a colour in 8-bit codes")
    return (*vals[:4], colour)


def check_crop(crop, crop_tol, height, width):
    """run_one_point's crop / crop_tol -> (None | 'auto' | the bars.ActiveArea of a manual crop, tol as the kernels take it:
    crop_tol 8-bit codes as repeat.tol_fraction turns them)"""
    tol = tol_fraction(crop_tol, "crop_tol")
    if tol and crop != "auto":
        raise ValueError(f"crop_tol {crop_tol!r} is the tolerance of crop='auto': it has no effect on crop {crop!r}")
    if crop is None or crop == "auto":
        return crop, tol
    from .bars import ActiveArea
    if isinstance(crop, str):
        crop = parse_crop(crop)
    if len(crop) != 5 or len(crop[4]) != 3:
        raise ValueError(f"crop {crop!r}: None, 'auto' or (top, bottom, left, right, (y, u, v))")
    colour = [float(np.float32(c) / np.float32(255.0)) for c in crop[4]]
    return ActiveArea.from_manual(height, width, crop[:4], colour), tol


def check_dup(frame_dup, dup_tol):
    """run_one_point's frame_dup / dup_tol: ValueError for a dup_tol that repeat.tol_fraction refuses or that is set without frame_dup"""
    if tol_fraction(dup_tol, "dup_tol") and not frame_dup:
        raise ValueError(f"dup_tol {dup_tol!r} is the tolerance of frame_dup: it has no effect without it")


def _detect_area(src, frame_num, dev, dtype, tol):
    """--crop auto: every frame of the run through the loader into one bars.BarDetector envelope, then ONE read-back ->
    the bars.ActiveArea to code, or None.  With the envelope over all frames and tol 0 no content can lie outside it."""
    from .bars import ActiveArea, BarDetector
    size = (src.h, src.w)
    det = BarDetector(dev)
    det.reset(size)
    reader = src.reader()
    for _ in range(frame_num):
        det.scan(src.to_input(_to_device(reader.read(), dev), dtype), size)
    reader.close()
    return ActiveArea.from_extents(*size, det.extents(tol))


def _front_input(src, planes, dtype, deint=None, area=None):
    """one source frame as the front end is fed it: loader -> deint (a deinterlace.Deinterlacer): its filter on the FULL frame, so
    that a crop's odd top offset can never flip the parity -> area (a bars.ActiveArea): its window.  What is None is off"""
    x = src.to_input(planes, dtype)
    if deint is not None:
        x = deint.filter(x, (src.h, src.w))
    return _windowed(src, x, area)


def _windowed(src, x, area):
    if area is not None:
        from .bars import window
        x = window(x, (src.h, src.w), area)
    return x


def _field_rate(deint):
    """is deint a Deinterlacer that makes two pictures per frame (docs/deinterlace.md, "Field-rate output")"""
    return getattr(deint, "rate", None) == "field"


def _reference_planes(src, planes, dtype, deint=None):
    """the planes a decoded frame is measured against: the source's own, or in a deinterlacing run (deint: a Deinterlacer of the
    decode pass's own, fed every source frame in order) the deinterlaced picture as a file of the source's format would hold it"""
    if deint is None:
        return planes
    return src.stored(deint.filter(src.to_input(planes, dtype), (src.h, src.w)))


def _references(src, reader, frame_num, dev, dtype, deint=None):
    """the reference planes of every picture the decode pass is to meet, in order, each made when it is asked for: one per source
    frame (_reference_planes), or at field rate the two pictures of every frame - deint.fields() per frame read, deint.drain()
    behind the last - as files of the source's format would hold them"""
    if not _field_rate(deint):
        for _ in range(frame_num):
            yield _reference_planes(src, _to_device(reader.read(), dev), dtype, deint)
        return
    for _ in range(frame_num):
        for pic in deint.fields(src.to_input(_to_device(reader.read(), dev), dtype), (src.h, src.w)):
            yield src.stored(pic)
    for pic in deint.drain():
        yield src.stored(pic)


def _encode_pass(nets, src, frame_num, dev, coded, scale_filter, grain, enc_kw, tf_level=0, tf_radius=2, tf_subpel=0,
                 lookahead=0, area=None, dup_tol=None, deint=None):
    """every frame of `src` through a frontend.FrontEnd into the container -> a frontend.EncodePass.  A frame goes loader -> deint
    (a deinterlace.Deinterlacer, made by the caller, who reads its counts afterwards): its filter, on the frame's clock -> area
    (a bars.ActiveArea): its window, whose size all behind it works at -> dup_tol (None: off; else 8-bit codes): a
    repeat.RepeatDetector -> tf_level 1 .. 5 or "auto": a prefilter.TemporalFilter tf_radius frames deep -> coded (height, width):
    the down-resample -> lookahead N > 0: a lookahead.Lookahead N frames deep -> SequenceEncoder(**enc_kw) -> write_frame; what is
    off is not made.  grain: None, a GrainParams, or "auto": estimated at every I frame from the UNFILTERED input of the frame being
    coded against the reconstruction at that size, seeded with the count of frames written so far.  A frame's clock: frontend.py.
    A field-rate deint gives the front end TWO pictures per frame read - fields()'s, then drain()'s behind the last read - and
    everything behind it counts pictures: the first picture of a read starts its clock at the read, every further one,
    drain()'s included, when it is made or handed over."""
    import torch
    from .frontend import EncodePass, FrontEnd
    from .grain import FilmGrain
    from .resize import Resampler
    size = area.size if area is not None else (src.h, src.w)
    dtype, (ch, cw) = next(nets[1].parameters()).dtype, coded or size
    sync, clock = (lambda: torch.cuda.synchronize(dev)), time.time
    scaler, grainer = Resampler(dev) if coded else None, FilmGrain(dev) if grain is not None else None
    if grain is not None:
        def estimate(x_coded, x_hat):
            x_hat = scaler.resample(x_hat, (ch, cw), size, scale_filter) if scaler else x_hat
            return grainer.estimate(front.coding.source, x_hat, size, len(front.units))
        enc_kw = dict(enc_kw, grain=estimate if grain == "auto" else grain)
    enc = SequenceEncoder(*nets, **enc_kw)
    det = tf = la = None
    if dup_tol is not None:                              # (the loader and the window allocate their output per frame: the
        from .repeat import RepeatDetector               # detector's reference is never overwritten, nothing is cloned for it)
        det = RepeatDetector(dev, dup_tol)
    if tf_level:
        from .prefilter import TemporalFilter
        tf = TemporalFilter(dev, tf_level, tf_radius, tf_subpel)
    if lookahead:
        from .lookahead import Lookahead
        la = Lookahead(dev, lookahead, enc.scenecut)
    out = io.BytesIO()
    writer = StreamWriter(out, display=size + (scale_filter,) if coded else None, active=area)
    front = FrontEnd(enc, writer, (ch, cw, use_two_entropy_coders(ch, cw)), sync, clock, size, det, tf,
                     (lambda x: scaler.resample(x, size, (ch, cw), scale_filter)) if scaler else None, la)

    field_rate = _field_rate(deint)
    reader = src.reader()
    for _ in range(frame_num):
        planes = _to_device(reader.read(), dev)
        sync()
        t0 = clock()
        if not field_rate:
            front.feed(_front_input(src, planes, dtype, deint, area), t0)
            continue
        for k, pic in enumerate(deint.fields(src.to_input(planes, dtype), (src.h, src.w))):
            if k:
                sync()
                t0 = clock()
            front.feed(_windowed(src, pic, area), t0)
    if field_rate:                                       # the last frame's second picture: its launch is on its own clock
        sync()
        t0 = clock()
        for pic in deint.drain():
            front.feed(_windowed(src, pic, area), t0)
    front.flush()
    reader.close()
    frame_types, bits, times, repeated = ([unit[i] for unit in front.units] for i in range(4))
    return EncodePass(enc, out.getvalue(), frame_types, bits, times, scaler, grainer, tf, la, repeated if det is not None else None)


def _decode_pass(nets, src, stream, frame_num, dev, calc_ssim, device_metrics, rec_path, scaler, grainer, deint=None):
    """the container back through a StreamDecoder, frame by frame against the source: metrics of the decoded picture,
    rec_path gets the shown one.  The clock of a frame spans the container read, the decoder's work, the synchronisation and
    the digest check.  deint: in a deinterlacing run a Deinterlacer of this pass's own - the metrics are then against
    _reference_planes, outside the clock; at field rate there are two of them per source frame, and as many pictures are
    decoded as there are references (_references).  -> (decoder, times, psnrs, ssims)"""
    import torch
    dtype = next(nets[1].parameters()).dtype if deint is not None else None
    reader = src.reader()
    decoder = StreamDecoder(io.BytesIO(stream), *nets, dev, scaler=scaler, grainer=grainer)
    src.open_rec(rec_path)
    dm = None
    if device_metrics:
        from .metrics import DeviceMetrics
        dm = DeviceMetrics(dev)
    times, psnrs, ssims = [], [], []
    for fi, planes in enumerate(_references(src, reader, frame_num, dev, dtype, deint)):
        torch.cuda.synchronize(dev)
        t0 = time.time()
        frame = decoder.next()
        shown_size = (src.h, src.w)                                                  # the stream's word, not the arguments'
        if frame.active is not None:
            if frame.active.full_size != shown_size:
                raise ValueError(f"the stream's full picture {frame.active.full_width}x{frame.active.full_height} is not the "
                                 f"source's {src.w}x{src.h}")
            shown_size = frame.active.size
        if frame.display is not None and frame.display[:2] != shown_size:
            raise ValueError(f"the stream's display size {frame.display[1]}x{frame.display[0]} is not the source's "
                             f"{shown_size[1]}x{shown_size[0]}")
        torch.cuda.synchronize(dev)
        decoder.check_digests()
        times.append(time.time() - t0)
        psnr, ssim = src.distortion(frame.x_hat, planes, calc_ssim, dm)
        psnrs.append(psnr)
        ssims.append(ssim)
        src.write_rec(frame.shown, fi)
    reader.close()
    src.close_rec()
    return decoder, times, psnrs, ssims


def _rate_log(enc, target, frame_num, frame_pixel_num, per_frame):
    """rate control's part of a point's log: rc_est_bpp is the mean of what the controller was fed, to hold against ave_all_frame_bpp"""
    log = {"target_bpp": target, "rc_qp": float(np.mean(enc.rc_qp)),
           "rc_est_bpp": float(8 * np.sum(enc.rc_est_bytes) / (frame_num * frame_pixel_num))}
    if per_frame:
        log["frame_rc_qp"] = [int(q) for q in enc.rc_qp]
        log["frame_rc_est_bpp"] = [8 * b / frame_pixel_num for b in enc.rc_est_bytes]
    return log


def run_one_point(i_net, p_net, src_path, width, height, frame_num, qp_i, qp_p=None, intra_period=-1,
                  reset_interval=32, bin_path=None, rec_path=None, verbose=0, verbose_json=False, device="cuda:0",
                  src_type="yuv420", calc_ssim=False, metrics="host", entropy="host", scenecut=0, min_keyint=4,
                  target_bpp=None, digest=False, coded_size=None, scale_filter="lanczos3", film_grain=None,
                  temporal_filter=0, tf_radius=2, tf_subpel=0, lookahead=0, crop=None, crop_tol=0.0, frame_dup=False,
                  dup_tol=0.0, deint_rate=None, deinterlace=None, field_order="tff"):
    # (deint_rate stands in FRONT of deinterlace / field_order, not behind them where it was added: tests/test_deint_host.py pins
    # those two as the last names.  Every option from device on is meant to be given by keyword, and every caller here does)
    """Encodes `frame_num` frames of a source (src_type: SRC_TYPES - a planar 8-bit YUV 4:2:0 file, a directory of PNGs, a raw
    file in a pipeline.PIXEL_FORMATS format) into the reference's container (optionally written to bin_path), decodes the
    container again and returns the reference-schema log (summarize) plus one group of keys per extension switched on.
    i_net / p_net: DMCI / DMC ready to code on `device`.  rec_path: the decoded sequence in the source's format / as PNGs in
    that directory.  Every argument error is raised before a net, a file or the device is touched.
      verbose >= 1                 avg_frame_encoding_time / avg_frame_decoding_time over the frames behind the first ten
      verbose_json, calc_ssim      summarize: per-frame lists; MS-SSIM instead of zeros (slow on the host)
      metrics, entropy             "host" | "device": torch glue + numpy / scipy or metrics.DeviceMetrics; docs/chunked_stream.md
      scenecut, min_keyint         pipeline.SequenceEncoder (scenecut)        log: scene_cuts
      target_bpp                   pipeline.SequenceEncoder (rate)            log: target_bpp, rc_qp, rc_est_bpp [, frame_rc_*]
      digest                       docs/state_digest.md                       log: digests_checked
      coded_size, scale_filter     docs/reduced_resolution.md                 log: coded_height, coded_width, scale_filter
      film_grain                   docs/film_grain.md (None, "auto", a GrainParams)   log: grain_units, grain_scale_y, grain_corr
      temporal_filter, tf_radius   docs/temporal_filter.md (level 0 = off .. 5; 1, 2)  log: tf_level, tf_radius, tf_mean_weight
                                   level "auto": chosen per frame from a noise estimate   log: + tf_levels, tf_noise
      tf_subpel                    its vectors in whole (0), half (1) or quarter pels (2)     log: + tf_subpel where not 0
      lookahead                    docs/lookahead.md (0 = off .. 16 frames; needs scenecut)   log: lookahead, flashes, fades
      crop, crop_tol               docs/active_area.md (None, "auto", (top, bottom, left, right, (y, u, v)) or its --crop spelling;
                                   the colour and crop_tol in 8-bit codes)             log: active_area, bar_colour
      frame_dup, dup_tol           docs/frame_repeat.md (a frame within dup_tol 8-bit codes of the last coded frame is sent as a
                                   one-byte repeat unit; bpp, target_bpp and the metrics stay per source frame, a repeat counts
                                   as a P frame)                                        log: repeat_frames, dup_tol [, frame_repeat]
      deinterlace, field_order     docs/deinterlace.md (None, "on", "auto", "film"; "tff", "bff": the field that is kept).  The source's
                                   frames are deinterlaced on the device in front of everything else, the crop included; PSNR /
                                   MS-SSIM are then against the DEINTERLACED source, quantised to the source's format - not
                                   against the woven frames               log: deinterlace, field_order, deint_frames
                                   "film": telecined film - a frame whose fields fit passes, one whose kept field fits the
                                   previous frame's other field is woven from the two, the rest is filtered; with frame_dup
                                   the repeated pictures of the pulldown become repeat units     log: + field_matches
      deint_rate                   None / "frame": a picture per source frame.  "field" (deinterlace "on" only): TWO pictures per
                                   source frame, one per field - 50i becomes 50p.  frame_num stays the count of SOURCE frames; the
                                   run codes and decodes 2 * frame_num pictures, and everything behind the filter - intra_period,
                                   reset_interval, min_keyint, lookahead, tf_radius, frame_dup, the digests, target_bpp, the
                                   per-frame lists - counts pictures           log: + deint_rate; deint_frames: the pictures"""
    from .deinterlace import check_deinterlace, check_height, check_rate
    from .grain import GrainParams
    from .lookahead import check_depth
    from .prefilter import check_options, check_subpel
    from .resize import FILTERS, check_coded_size
    for name, value, choices in (("metrics", metrics, ("host", "device")), ("entropy", entropy, ("host", "device")),
                                 ("src_type", src_type, SRC_TYPES + SRC_TYPES_422), ("scale_filter", scale_filter, FILTERS)):
        if value not in choices:
            raise ValueError(f"{name} {value!r}: one of {', '.join(choices)}")
    area, tol = check_crop(crop, crop_tol, height, width)
    check_dup(frame_dup, dup_tol)
    deinterlace, _ = check_deinterlace(deinterlace, field_order)
    field_rate = check_rate(deint_rate, deinterlace) == "field"
    coded_size = check_coded_size(coded_size, *(area.size if area not in (None, "auto") else (height, width)))
    if not (film_grain is None or film_grain == "auto" or isinstance(film_grain, GrainParams)):
        raise ValueError(f"film_grain {film_grain!r}: None, 'auto' or a GrainParams")
    temporal_filter, tf_radius = check_options(temporal_filter, tf_radius)
    tf_subpel = check_subpel(tf_subpel)
    if check_depth(lookahead) and not scenecut:
        raise ValueError("lookahead decides the scene cuts of scenecut: give scenecut too")
    src = make_source(src_type, src_path, width, height)
    if deinterlace:
        check_height(height, src.chroma_lines, f"deinterlace of a {src_type} source")
    import torch
    dev, nets = torch.device(device), (i_net, p_net)
    t_start = time.time()
    if area == "auto":               # a pass of its own over every frame of the run, outside the per-frame clocks
        area = _detect_area(src, frame_num, dev, next(p_net.parameters()).dtype, tol)
        if area is not None:
            coded_size = check_coded_size(coded_size, *area.size)
    for m in nets:
        m.set_use_two_entropy_coders(use_two_entropy_coders(*(coded_size or (area.size if area else (height, width)))))     # what the SPS and the models see
        m.entropy = entropy
    enc_kw = dict(qp_i=qp_i, qp_p=qp_p, intra_period=intra_period, reset_interval=reset_interval)
    if scenecut:
        enc_kw.update(scenecut=scenecut, min_keyint=min_keyint)
    if target_bpp:
        from .ratecontrol import RateController
        enc_kw["rate"] = RateController(float(target_bpp) * height * width, qp_i if qp_p is None else qp_p, qp_i_init=qp_i)
    else:
        i_net.rate_estimate = p_net.rate_estimate = False       # (one pair codes every point)
    if digest:
        enc_kw["digest"] = True
    extra = dict({"tf_subpel": tf_subpel} if tf_subpel else {}, **({"lookahead": lookahead} if lookahead else {}))
    if area is not None:
        extra["area"] = area
    if frame_dup:
        extra["dup_tol"] = dup_tol
    dec_extra = {}
    if deinterlace:                  # one for each pass: the same frames in the same order, the same pictures and decisions
        from .deinterlace import Deinterlacer
        rate = ("field",) if field_rate else ()          # (frame rate: the call of before the option)
        extra["deint"], dec_extra["deint"] = (Deinterlacer(dev, deinterlace, field_order, src.chroma_lines, *rate) for _ in range(2))
    done = _encode_pass(nets, src, frame_num, dev, coded_size, scale_filter, film_grain, enc_kw, temporal_filter, tf_radius, **extra)
    picture_num = 2 * frame_num if field_rate else frame_num
    coded_num = picture_num - sum(done.repeated) if frame_dup else picture_num     # the pictures the filter and the encoder saw
    if bin_path:
        with open(bin_path, "wb") as f:
            f.write(done.stream)
    decoder, dec_time, psnrs, ssims = _decode_pass(nets, src, done.stream, frame_num, dev, calc_ssim, metrics == "device", rec_path,
                                                   done.scaler, done.grainer, **dec_extra)
    test_time = time.time() - t_start
    timed = verbose >= 1 and frame_num > 10     # the first 10 frames are warm-up (test_video.py:328-333)
    log = summarize(height * width, test_time, done.frame_types, done.bits, psnrs, ssims, verbose=verbose_json,
                    avg_encoding_time=sum(done.times[10:]) / len(done.times[10:]) if timed else None,
                    avg_decoding_time=sum(dec_time[10:]) / len(dec_time[10:]) if timed else None)
    if scenecut:
        log["scene_cuts"] = list(done.enc.scene_cuts)
    if done.lookahead is not None:
        log.update(lookahead=lookahead, flashes=list(done.lookahead.flashes), fades=list(done.lookahead.fades))
    if target_bpp:
        log.update(_rate_log(done.enc, float(target_bpp), picture_num, height * width, verbose_json))
    if digest:
        log["digests_checked"] = decoder.digests_checked
    if coded_size:
        log["coded_height"], log["coded_width"], log["scale_filter"] = *coded_size, scale_filter
    if film_grain is not None:
        last = done.enc.grain_units[-1] if done.enc.grain_units else None
        log.update(grain_units=len(done.enc.grain_units), grain_scale_y=list(last.scale_y) if last else [],
                   grain_corr=last.corr if last else 0)
    if done.tf is not None:
        log.update(tf_level=temporal_filter, tf_radius=tf_radius,
                   tf_mean_weight=done.tf.weight_sum() / (256.0 * (area.height * area.width if area else height * width) * coded_num))
        if temporal_filter == "auto":                     # frames per level 0 .. 5; the mean N as white noise's sigma in 8-bit codes
            totals = done.tf.levels()
            log.update(tf_levels=totals[:6], tf_noise=totals[6] / max(totals[7], 1) * (255.0 / (68.0 * 1023.0)))
        if tf_subpel:
            log["tf_subpel"] = tf_subpel
    if crop is not None:
        log["active_area"] = area.extents if area is not None else [0, 0, 0, 0]
        log["bar_colour"] = list(area.colour) if area is not None else None
    if frame_dup:
        log.update(repeat_frames=sum(done.repeated), dup_tol=float(dup_tol))
        if verbose_json:
            log["frame_repeat"] = list(done.repeated)
    if deinterlace == "film":        # one read-back of the four device counters
        passed, woven, filtered = extra["deint"].matches()
        log.update(deinterlace=deinterlace, field_order=field_order, deint_frames=filtered,
                   field_matches={"pass": passed, "weave": woven})
    elif deinterlace:
        log.update(deinterlace=deinterlace, field_order=field_order, **({"deint_rate": "field"} if field_rate else {}),
                   deint_frames=extra["deint"].filtered())
    return log


# The per-point options: (run_one_point keyword, default, normaliser of a value that is set or None).  run_job, main and
# manifest_options all go through point_kwargs, so a new option is one row here, one build_parser line under the same name and
# its hook in run_one_point.  target_bpp is not one of them: it is worked out per sequence (target_bpp()).  Nor
# are temporal_filter / tf_radius / tf_subpel: they act in front of the encoder, not on a rate point, and the table's names are pinned
# (tests/test_harness_options.py), so they travel target_bpp's way - prefilter_kwargs(), passed beside point_kwargs().  lookahead goes the same way: lookahead_kwargs().  So does crop / crop_tol: crop_kwargs(), which hands on nothing at all where the option is not set, and frame_dup / dup_tol: dup_kwargs(), likewise, and deinterlace / field_order / deint_rate: deint_kwargs().
POINT_OPTIONS = (("verbose", 0, None), ("verbose_json", False, bool), ("calc_ssim", False, bool), ("metrics", "host", None),
                 ("entropy", "host", None), ("scenecut", 0, None), ("min_keyint", 4, None), ("digest", False, bool),
                 ("coded_size", None, None), ("scale_filter", "lanczos3", None), ("film_grain", None, None))


def point_kwargs(opts):
    """an options mapping (a manifest run's opts, vars() of the parsed command line) -> run_one_point's keywords of
    POINT_OPTIONS; an option that is missing, None or otherwise false takes its default"""
    return {name: (norm or (lambda v: v))(opts.get(name) or default) for name, default, norm in POINT_OPTIONS}


def prefilter_kwargs(opts):
    """an options mapping -> run_one_point's keywords of the temporal pre-filter; missing or None: the defaults (off, radius 2);
    tf_subpel only where it is set and not 0 (whole-pel vectors: the keywords of before the option)"""
    level, radius = opts.get("temporal_filter"), opts.get("tf_radius")
    kw = {"temporal_filter": 0 if level is None else level, "tf_radius": 2 if radius is None else radius}
    if opts.get("tf_subpel"):
        kw["tf_subpel"] = opts["tf_subpel"]
    return kw


def lookahead_kwargs(opts):
    """an options mapping -> run_one_point's keyword of the frame lookahead; missing or None: 0, off.  Like the pre-filter's it
    acts in front of the encoder and travels beside point_kwargs()"""
    return {"lookahead": opts.get("lookahead") or 0}


def crop_kwargs(opts):
    """an options mapping -> run_one_point's keywords of active-area coding: none at all where crop is missing or None (the
    keywords of before the option), crop_tol only where it is set and not 0.  Like the pre-filter's it acts in front of the
    encoder and travels beside point_kwargs()"""
    if not opts.get("crop"):
        return {}
    return dict({"crop": opts["crop"]}, **({"crop_tol": opts["crop_tol"]} if opts.get("crop_tol") else {}))


def dup_kwargs(opts):
    """an options mapping -> run_one_point's keywords of repeated-frame coding: none at all where frame_dup is missing or
    false (the keywords of before the option), dup_tol only where it is set and not 0.  It acts in front of the encoder and
    travels beside point_kwargs(), as crop_kwargs() does"""
    if not opts.get("frame_dup"):
        return {}
    return dict({"frame_dup": True}, **({"dup_tol": opts["dup_tol"]} if opts.get("dup_tol") else {}))


def deint_kwargs(opts):
    """an options mapping -> run_one_point's keywords of deinterlacing: none at all where deinterlace is missing or None (the
    keywords of before the option), field_order and deint_rate only where they are set.  It acts in front of the encoder and
    travels beside point_kwargs(), as crop_kwargs() does"""
    if not opts.get("deinterlace"):
        return {}
    return dict({"deinterlace": opts["deinterlace"]}, **{k: opts[k] for k in ("field_order", "deint_rate") if opts.get(k)})


def run_sweep(make_nets, src_path, width, height, frame_num, rate_num=4, qp_i=None, qp_p=None, bin_prefix=None, **kw):
    """RD points of one sequence (test_video.py:448-463 + the per-point loop :472-510): {qp_i: log}.
    make_nets() -> (i_net, p_net) ready to use; one pair codes every point, like a reference worker.
    bin_prefix: write each point's container to <prefix>_q<qp_i>.bin (the reference's naming, test_video.py:367)."""
    qi = list(qp_i) if qp_i is not None else sweep_qps(rate_num)
    qp = list(qp_p) if qp_p is not None else qi
    i_net, p_net = make_nets()
    out = {}
    for q, qq in zip(qi, qp):
        out[q] = run_one_point(i_net, p_net, src_path, width, height, frame_num, q, qq,
                               bin_path=f"{bin_prefix}_q{q}.bin" if bin_prefix else None, **kw)
        out[q].update(qp_i=q, qp_p=qq)          # the keys test_video.worker adds to a point's result (:373-376)
    return out


# ---------------------------------------------------------------------------------- job fan-out (test_video.py main)
def dump_json(obj, fp, float_digits=6, indent=2):
    """The reference's log writer (common.py:49-60): json.dump with every float printed with `float_digits` digits."""
    enc = json.JSONEncoder(indent=indent)
    it = json.encoder._make_iterencode({}, enc.default, json.encoder.encode_basestring_ascii, " " * indent,
                                       lambda o: format(o, ".%df" % float_digits), enc.key_separator, enc.item_separator,
                                       enc.sort_keys, enc.skipkeys, False)
    for chunk in it(obj, 0):
        fp.write(chunk)


def jobs_from_config(config, opts):
    """One job per (dataset, sequence, rate point), in the reference's submission order (test_video.py:472-510).
    config: the parsed dataset manifest (dataset_config_example_yuv420.json); opts: see run_config()."""
    qi = list(opts["qp_i"]) if opts.get("qp_i") else sweep_qps(opts.get("rate_num", 4))
    qp = list(opts["qp_p"]) if opts.get("qp_p") else qi
    assert len(qi) == len(qp)
    root = opts.get("force_root_path") or config["root_path"]
    jobs = []
    for ds_name, ds in config["test_classes"].items():
        if ds["test"] == 0:
            continue
        if ds["src_type"] not in SRC_TYPES + SRC_TYPES_422:
            raise ValueError(f"{ds_name}: src_type {ds['src_type']!r} (one of {', '.join(SRC_TYPES + SRC_TYPES_422)})")
        for seq, info in ds["sequences"].items():
            for rate_idx, (q, qq) in enumerate(zip(qi, qp)):
                ip = info["intra_period"]
                if opts.get("force_intra"):                      # every frame an I frame (test_video.py:490-491)
                    ip = 1
                if opts.get("force_intra_period", 0) > 0:
                    ip = opts["force_intra_period"]
                fn = opts["force_frame_num"] if opts.get("force_frame_num", 0) > 0 else info["frames"]
                jobs.append(dict(ds_name=ds_name, seq=seq, rate_idx=rate_idx, qp_i=q, qp_p=qq,
                                 src_path=os.path.join(root, ds["base_path"], seq), src_width=info["width"],
                                 src_height=info["height"], frame_num=fn, intra_period=ip,
                                 reset_interval=opts.get("reset_interval", 32), src_type=ds["src_type"]))
    return jobs


def merge_results(config, results):
    """{dataset: {sequence: {"000": result, "001": ...}}} (test_video.py:517-528)"""
    log = {}
    for ds_name, ds in config["test_classes"].items():
        if ds["test"] == 0:
            continue
        log[ds_name] = {seq: {} for seq in ds["sequences"]}
    for res in results:
        log[res["ds_name"]][res["seq"]][f"{res['rate_idx']:03d}"] = res
    return log


_WORKER = {}


def worker_gpu(process_name, gpu_num):
    """test_video.py:384-388: worker process n (the number at the end of its multiprocessing name) codes on GPU
    n % gpu_num; -1 without GPUs."""
    idx = int(process_name[process_name.rfind("-") + 1:])
    return idx % gpu_num if gpu_num > 0 else -1


MIN_WORKER_CPUS = 3      # codec thread + the two rANS worker threads of a 1080p stream


def worker_cpus(idx, workers, allowed, quota=None):
    """CPU set of pool worker `idx` of `workers`: its contiguous slice of the allowed CPUs; with a cgroup quota below the
    mask only as many CPUs of the slice as its share of the quota is worth (spreading wider buys no CPU time) - but never
    fewer than MIN_WORKER_CPUS (neighbouring workers then share some)."""
    n = len(allowed)
    lo, hi = idx * n // workers, (idx + 1) * n // workers
    if quota is not None:
        hi = min(hi, lo + max(MIN_WORKER_CPUS, quota // workers))
    if hi - lo < MIN_WORKER_CPUS:
        lo = max(0, min(lo, n - MIN_WORKER_CPUS))
        hi = min(n, lo + MIN_WORKER_CPUS)
    return allowed[lo:hi] or allowed


def visible_gpu_ids(env=None):
    """The physical device ids the parent process was given (HIP_VISIBLE_DEVICES / ROCR_VISIBLE_DEVICES /
    CUDA_VISIBLE_DEVICES, a scheduler's assignment), in order; None if none is set.  Workers index THIS list
    (the reference's --cuda_idx, test_video.py:389-393) - worker n must not land on physical GPU n when the job was
    given GPUs 4,5."""
    env = os.environ if env is None else env
    for var in ("HIP_VISIBLE_DEVICES", "ROCR_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"):
        v = env.get(var)
        if v:
            ids = [t.strip() for t in v.split(",") if t.strip()]
            if ids:
                return ids
    return None


def count_gpus():
    """number of AMD GPUs the workers may use, without a HIP call in the parent: the visible-devices list if there is
    one, else the render nodes in sysfs"""
    ids = visible_gpu_ids()
    if ids is not None:
        return len(ids)
    from . import dist
    return len(dist.gpu_local_cpus())


def _init_worker(opts, gpu_num):
    """Runs once in every spawned worker (test_video.py:381-414): picks the GPU, pins the process, loads both models."""
    import multiprocessing
    gpu = worker_gpu(multiprocessing.current_process().name, gpu_num)
    if gpu >= 0:
        ids = opts.get("gpu_ids")
        os.environ["HIP_VISIBLE_DEVICES"] = str(ids[gpu] if ids else gpu)     # before the first GPU call of the process
    workers_here = max(1, opts.get("workers", 1))
    try:
        # Every worker stays on its slice of the allowed CPUs, never on fewer than MIN_WORKER_CPUS of them: a worker runs the
        # codec thread plus two rANS worker threads, and a cgroup cpu.max quota limits CPU TIME, not parallelism - cutting a
        # slice down to quota // workers (one CPU at -w 16 on a 16-CPU grant) would put the host coder behind the kernel
        # launches it is meant to overlap.  Slices of neighbouring workers overlap when there are fewer CPUs than that.
        from . import dist
        idx = (int(multiprocessing.current_process().name.rsplit("-", 1)[1]) - 1) % workers_here
        os.sched_setaffinity(0, worker_cpus(idx, workers_here, sorted(os.sched_getaffinity(0)), dist.cgroup_cpu_quota()))
    except (OSError, ValueError, ImportError):
        pass
    mod, fn = opts.get("codec", "opendcvc_amd.harness:default_nets").split(":")
    _WORKER["gpu"] = gpu
    _WORKER["nets"] = getattr(importlib.import_module(mod), fn)(opts)
    mod, fn = opts.get("runner", "opendcvc_amd.harness:run_job").split(":")
    _WORKER["run"] = getattr(importlib.import_module(mod), fn)
    _WORKER["opts"] = opts


def load_nets(model_i, model_p, force_zero_thres, fp32, device):
    """(DMCI, DMC) ready to code on `device`: checkpoints if given (reference keys, a DataParallel "module." prefix dropped),
    else the synthetic weights; fp16 like the reference harness unless fp32."""
    import torch
    from . import weights
    from .models import DMC, DMCI
    nets = []
    for cls, name, path in ((DMCI, "dmci", model_i), (DMC, "dmc", model_p)):
        m = cls()
        if path:
            ck = torch.load(path, map_location="cpu", weights_only=True)
            ck = ck.get("state_dict", ck)
            ck = ck.get("net", ck)
            m.load_state_dict({k[7:] if k.startswith("module.") else k: v for k, v in ck.items()})
        else:
            m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in
                               weights.make_state_dict(name, 1234).items()})
        m.to(device).eval()
        m.update(force_zero_thres)
        if not fp32:
            m.half()
        nets.append(m)
    return nets


def default_nets(opts):
    """load_nets of a worker's options, on cuda:0 of the worker (its HIP_VISIBLE_DEVICES names one GPU)"""
    import torch
    torch.set_num_threads(1)          # src/utils/common.py:23
    return load_nets(opts.get("model_i"), opts.get("model_p"), opts.get("force_zero_thres", 0.12), opts.get("fp32"), "cuda:0")


def run_job(nets, job, opts):
    """one (sequence, rate point) on this worker's GPU -> the reference-schema log of the point (test_video.py:354-379 worker +
    :130-137, 251-255, 345-346): with a stream folder the point's container <stream_path>/<dataset>/<sequence>_q<qp>.bin and its log
    <...>.json are written; check_existing returns the stored log of a point whose container and log exist with the right
    frame count instead of coding it again; save_decoded_frame writes the reconstruction beside them (<...>.yuv, or PNGs in
    the dataset's stream folder for PNG sources)."""
    bin_path = json_path = rec_path = None
    if opts.get("stream_path"):
        folder = os.path.join(opts["stream_path"], job["ds_name"])
        os.makedirs(folder, exist_ok=True)
        bin_path = os.path.join(folder, f"{job['seq']}_q{job['qp_i']}.bin")         # test_video.py:364-367
        json_path = bin_path[:-4] + ".json"
        if opts.get("save_decoded_frame"):
            rec_path = folder if job.get("src_type") == "png" else bin_path[:-4] + ".yuv"
        if opts.get("check_existing") and os.path.exists(json_path) and os.path.exists(bin_path):
            with open(json_path) as f:
                log = json.load(f)
            pictures = job["frame_num"] * (2 if opts.get("deint_rate") == "field" else 1)      # field rate: two per frame
            if log.get("i_frame_num", 0) + log.get("p_frame_num", 0) == pictures:
                return log
            print(f"incorrect log for {json_path}, try to rerun.")
    log = run_one_point(nets[0], nets[1], job["src_path"], job["src_width"], job["src_height"], job["frame_num"],
                        job["qp_i"], job["qp_p"], intra_period=job["intra_period"], reset_interval=job["reset_interval"],
                        bin_path=bin_path, rec_path=rec_path, device="cuda:0", src_type=job.get("src_type", "yuv420"),
                        target_bpp=target_bpp(opts, job["src_width"], job["src_height"]), **prefilter_kwargs(opts),
                        **lookahead_kwargs(opts), **crop_kwargs(opts), **dup_kwargs(opts), **deint_kwargs(opts),
                        **point_kwargs(opts))
    if json_path:
        with open(json_path, "w") as f:
            json.dump(log, f, indent=2)
    return log


def _worker(job):
    res = _WORKER["run"](_WORKER["nets"], job, _WORKER["opts"])
    res["ds_name"], res["seq"], res["rate_idx"] = job["ds_name"], job["seq"], job["rate_idx"]      # test_video.py:371-376
    res["qp_i"], res["qp_p"] = job["qp_i"], job["qp_p"]
    if _WORKER["opts"].get("record_gpu"):
        res["gpu"] = _WORKER["gpu"]
    return res


def run_config(config, opts, workers=1, gpus=1):
    """The reference's main loop (test_video.py:417-532): every (sequence, rate point) of the manifest as a job on a pool
    of `workers` spawned processes, worker n on GPU n % gpus (so -w may exceed the GPU count: two streams per GPU
    give ~16 % more frames/s on an MI355X, profiles/r02_multistream.txt); returns the merged log."""
    import concurrent.futures
    import multiprocessing
    jobs = jobs_from_config(config, opts)
    opts = dict(opts, workers=workers)
    ctx = multiprocessing.get_context("spawn")
    with concurrent.futures.ProcessPoolExecutor(max_workers=workers, mp_context=ctx, initializer=_init_worker,
                                                initargs=(opts, gpus)) as pool:
        results = [f.result() for f in [pool.submit(_worker, j) for j in jobs]]
    return merge_results(config, results)


def target_bpp(opts, width, height):
    """--target-bpp, or --target-kbps with --fps, as bits per pixel of a width x height sequence (None: no rate control).  Per
    coded picture: --fps is the SOURCE's frame rate, and at --deint-rate field a second carries twice as many pictures"""
    if opts.get("target_bpp"):
        return float(opts["target_bpp"])
    if opts.get("target_kbps"):
        pictures = 2.0 if opts.get("deint_rate") == "field" else 1.0
        return float(opts["target_kbps"]) * 1000.0 / (pictures * float(opts["fps"]) * width * height)
    return None


def check_rate_options(args, ap):
    if args.target_bpp is not None and args.target_kbps is not None:
        ap.error("--target-bpp and --target-kbps are two spellings of one target: give one")
    if (args.target_kbps is not None) != (args.fps is not None):
        ap.error("--target-kbps and --fps go together")
    if any(v is not None and not v > 0 for v in (args.target_bpp, args.target_kbps, args.fps)):
        ap.error("--target-bpp / --target-kbps / --fps must be positive")
    if args.target_bpp is None and args.target_kbps is None:
        return
    # one rate point: the controller chooses the qp, --qp-i / --qp-p (default 32) only say where it starts
    args.qp_i = list(args.qp_i)[:1] if args.qp_i else [32]
    args.qp_p = list(args.qp_p)[:1] if args.qp_p else list(args.qp_i)
    args.rate_num = 1


def check_lookahead_options(args, ap):
    if args.lookahead and not args.scenecut:
        ap.error("--lookahead decides the scene cuts of --scenecut: give --scenecut too (150 is recommended)")


def check_crop_options(args, ap):
    if args.crop_tol is not None and args.crop != "auto":
        ap.error("--crop-tol is the tolerance of --crop auto's bar detection: it has no effect without it")
    if args.crop_tol is not None and not args.crop_tol >= 0:
        ap.error("--crop-tol is in 8-bit codes, >= 0")


def check_dup_options(args, ap):
    if args.dup_tol is not None and not args.frame_dup:
        ap.error("--dup-tol is the tolerance of --frame-dup: it has no effect without it")
    if args.dup_tol is not None and not args.dup_tol >= 0:
        ap.error("--dup-tol is in 8-bit codes, >= 0")


def check_deint_options(args, ap):
    if args.field_order is not None and not args.deinterlace:
        ap.error("--field-order is the field order of --deinterlace: it has no effect without it")
    if args.deint_rate == "field" and args.deinterlace != "on":
        ap.error("--deint-rate field is the field-rate output of --deinterlace on: it cannot go with --deinterlace "
                 f"{args.deinterlace or 'unset'}")


def _str2bool(v):
    """the reference's str2bool (test_video.py:24-28): --flag 1 / true / yes / y / t"""
    if isinstance(v, bool):
        return v
    if str(v).lower() in ("yes", "y", "true", "t", "1"):
        return True
    if str(v).lower() in ("no", "n", "false", "f", "0"):
        return False
    raise ValueError("boolean value expected, got %r" % (v,))


def _add_extension_options(ap, flag):
    """this project's options beyond the reference's: adaptive I frames, rate control, digests, reduced resolution, film grain,
    the temporal pre-filter, the frame lookahead, active-area coding, repeated-frame coding, deinterlacing"""
    from .resize import FILTERS, parse_size
    ap.add_argument("--scenecut", type=int, default=0, metavar="PCT",
                    help="adaptive I frames: a frame whose low-resolution difference to its predecessor is at least PCT percent "
                         "of its own spatial activity starts a new GOP (0 = off, the reference's placement; 150 is recommended); "
                         "--intra-period and --reset-interval then count from the most recent I frame")
    ap.add_argument("--min-keyint", "--min_keyint", type=int, default=4, metavar="N",
                    help="with --scenecut: a cut fewer than N frames after the last I frame is coded as a P frame")
    ap.add_argument("--lookahead", type=int, default=0, choices=range(0, 17), metavar="N",
                    help="with --scenecut: decide every frame's cut with N more frames in view (0 = off, up to 16; 4 is "
                         "recommended): a flash, a fade and a pan no longer cost an I frame (docs/lookahead.md).  Encoder side "
                         "only, the stream format is unchanged; the encoder reads N frames ahead")
    ap.add_argument("--target-bpp", "--target_bpp", type=float, default=None, metavar="X",
                    help="target-bitrate control: aim at X bits per pixel (one rate point; --qp-i / --qp-p give the starting qp)")
    ap.add_argument("--target-kbps", "--target_kbps", type=float, default=None, metavar="K",
                    help="the same as a bitrate: K * 1000 / (--fps * width * height) bits per pixel, per sequence")
    ap.add_argument("--fps", type=float, default=None, metavar="F", help="frame rate of the source, for --target-kbps")
    ap.add_argument("--digest", **flag,
                    help="write a digest of the decoder's reference state in front of every frame and check it while decoding "
                         "(docs/state_digest.md) - this project's extension, not readable by the reference")
    ap.add_argument("--coded-size", "--coded_size", type=parse_size, default=None, metavar="WxH",      # (a malformed size: a usage error)
                    help="reduced-resolution coding: resample every frame down to W x H on the device, code that, and resample "
                         "the decoded frames back up; metrics, bpp and --target-bpp stay those of the source "
                         "(docs/reduced_resolution.md) - this project's extension, not readable by the reference")
    ap.add_argument("--scale-filter", "--scale_filter", choices=FILTERS, default="lanczos3",
                    help="the resampling filter of --coded-size, down and up")
    ap.add_argument("--film-grain", "--film_grain", nargs="?", const="auto", default=None,
                    type=lambda v: "auto" if v == "auto" or _str2bool(v) else None,
                    help="film-grain synthesis: at every I frame the grain the codec removed is estimated on the device and "
                         "written as a 14-byte grain unit; the decode loop puts it back on the pictures it stores, not on "
                         "the ones it measures (docs/film_grain.md) - this project's extension, not readable by the reference")
    ap.add_argument("--temporal-filter", "--temporal_filter", type=_tf_level, default=0, metavar="L",
                    help="motion-compensated temporal denoising of the source in front of the encoder at strength L = 1 .. 5 "
                         "(0 = off; 3 is recommended; docs/temporal_filter.md), or `auto`: the level is chosen per frame from "
                         "a noise estimate made on the device.  Encoder side only, the stream format is "
                         "unchanged.  The counterpart of --film-grain: the encoder stops spending bits on noise the decoder "
                         "synthesises anyway.  Metrics stay those against the unfiltered source")
    ap.add_argument("--tf-radius", "--tf_radius", type=int, default=2, choices=(1, 2), metavar="R",
                    help="with --temporal-filter: references up to R frames before and after a frame (the encoder reads R frames ahead)")
    ap.add_argument("--crop", type=parse_crop, default=None, metavar="auto|T:B:L:R[:Y:U:V]",
                    help="active-area coding: code only the picture between the black bars of letterboxed / pillarboxed "
                         "material and paste it back behind the decoder.  auto: the bars are found on the device in a pass over "
                         "every frame of the run; T:B:L:R: the rows / columns to leave out (even numbers), Y:U:V the bars' "
                         "colour in 8-bit codes (16:128:128).  Metrics, bpp and --target-bpp stay those of the source "
                         "(docs/active_area.md) - this project's extension, not readable by the reference")
    ap.add_argument("--crop-tol", "--crop_tol", type=float, default=None, metavar="X",
                    help="with --crop auto: a line is a bar while it stays within X 8-bit codes of the bars' colour (default 0: "
                         "exactly flat bars, nothing can be lost; above 0 for noisy bars)")
    ap.add_argument("--frame-dup", "--frame_dup", **flag,
                    help="repeated-frame coding: a frame that is the picture of the last coded frame (screen and slide capture, "
                         "animation on twos, 24 -> 30 fps conversions, frozen feeds) is found on the device and sent as a "
                         "one-byte repeat unit; the encoder sees the sequence without it (docs/frame_repeat.md) - this "
                         "project's extension, not readable by the reference")
    ap.add_argument("--dup-tol", "--dup_tol", type=float, default=None, metavar="X",
                    help="with --frame-dup: a frame is a repeat while every sample stays within X 8-bit codes of the last coded "
                         "frame (default 0: equal frames only; above 0 for material that went through a dithered stage)")
    ap.add_argument("--deinterlace", choices=("on", "auto", "film"), default=None,
                    help="the source is interlaced (1080i, DVD, archive material): every frame is deinterlaced on the device in "
                         "front of everything else - the first field's lines are kept, the second field's rebuilt from the "
                         "current and the previous frame, motion-adaptive and edge-directed, same frame rate "
                         "(docs/deinterlace.md).  auto: decided per frame on the device, a progressive frame passes bit for "
                         "bit.  film: telecined film - per frame the device finds the field that completes the first one, in the "
                         "same frame (it passes bit for bit) or in the previous one (the two are woven); a frame that matches "
                         "neither is filtered; with --frame-dup the pulldown's repeated pictures cost a byte each.  Encoder side only, the stream format is unchanged.  PSNR / MS-SSIM are then against the "
                         "deinterlaced source, quantised to the source's format")
    ap.add_argument("--field-order", "--field_order", choices=("tff", "bff"), default=None,
                    help="with --deinterlace: the field that comes first and is kept - tff: the even lines (default), bff: the odd ones")
    ap.add_argument("--deint-rate", "--deint_rate", choices=("frame", "field"), default=None,
                    help="with --deinterlace on: frame - one picture per source frame, the field that comes first (default); "
                         "field - TWO pictures per source frame, one per field, 50i becomes 50p: --frames stays the count of "
                         "source frames, twice as many pictures are coded and decoded, and --intra-period, --reset-interval, "
                         "--min-keyint, --lookahead, --tf-radius and --target-bpp count pictures; --fps stays the source's "
                         "frame rate (docs/deinterlace.md, \"Field-rate output\")")
    ap.add_argument("--tf-subpel", "--tf_subpel", type=int, default=0, choices=(0, 1, 2), metavar="S",
                    help="with --temporal-filter: refine the filter's motion vectors to half (1) or quarter pels (2) and gather "
                         "interpolated reference samples (0 = whole-pel vectors; 2 is recommended for camera material)")


def _tf_level(v):
    """--temporal-filter: 0 .. 5 as an int, or auto"""
    import argparse
    if v == "auto":
        return v
    try:
        level = int(v)
    except ValueError:
        level = -1
    if not 0 <= level <= 5:
        raise argparse.ArgumentTypeError(f"{v!r}: 0 .. 5 or auto")
    return level


def build_parser():
    """The command line.  Every option of the reference's test_video.py (parse_args, test_video.py:30-56) is accepted under
    its own spelling and value convention too (`--test_config`, `--model_path_i`, `--write_stream 1`, `--cuda_idx 0 1`, ...):
    the command of the reference's README runs unchanged as `python -m opendcvc_amd.harness ...`."""
    import argparse
    ap = argparse.ArgumentParser(description="DCVC-RT rate points of one YUV 4:2:0 sequence on the MI355X path")
    flag = dict(nargs="?", const=True, default=False, type=_str2bool)       # `--flag` or the reference's `--flag True`
    ap.add_argument("--test-config", "--test_config", help="JSON dataset manifest (reference: dataset_config_example_yuv420.json): every "
                    "sequence x rate point becomes a job on the worker pool (reference: test_video.py --test_config)")
    ap.add_argument("-w", "--worker", type=int, default=1, help="worker processes (may exceed --gpus)")
    ap.add_argument("--gpus", type=int, default=None, help="GPUs to spread the workers over (default: all visible)")
    ap.add_argument("--gpu-ids", type=lambda v: [t for t in v.split(",") if t], default=None,
                    help="physical device ids for the workers, comma separated (reference: --cuda_idx); default: the "
                         "parent's HIP_VISIBLE_DEVICES / ROCR_VISIBLE_DEVICES / CUDA_VISIBLE_DEVICES list, else 0..gpus-1")
    ap.add_argument("--cuda_idx", type=int, nargs="+", default=None, help="the reference's spelling of --gpu-ids: 0 1 2 ...")
    ap.add_argument("--cuda", **dict(flag, default=True), help="accepted for the reference's command line; there is no CPU path: "
                    "--cuda 0 is an error")
    ap.add_argument("--write_stream", "--write-stream", **flag, help="the reference's switch for writing the containers (to "
                    "--stream_path, default out_bin); here giving --stream-path is enough")
    ap.add_argument("--force-root-path", "--force_root_path")
    ap.add_argument("--force-frame-num", "--force_frame_num", type=int, default=-1)
    ap.add_argument("--force-intra-period", "--force_intra_period", type=int, default=-1)
    ap.add_argument("--stream-path", "--stream_path", help="write every point's container to <stream-path>/<dataset>/<sequence>_q<qp>.bin")
    ap.add_argument("--output-path", "--output_path", help="merged JSON log of the manifest run")
    ap.add_argument("--calc-ssim", "--calc_ssim", **flag, help="MS-SSIM per frame (reference --calc_ssim; host computation, slow)")
    ap.add_argument("--metrics", choices=("host", "device"), default="host",
                    help="where PSNR / MS-SSIM are computed: host (torch glue + numpy / scipy MS-SSIM) or device (HIP kernels)")
    ap.add_argument("--entropy", choices=("host", "device"), default="host",
                    help="host: the reference's stream format, host rANS coder.  device: chunked payloads entropy-coded by HIP "
                         "kernels - this project's extension, not readable by the reference")
    ap.add_argument("--force-intra", "--force_intra", **flag, help="every frame an I frame (reference --force_intra)")
    ap.add_argument("--check-existing", "--check_existing", **flag,
                    help="with --stream-path: do not code a point again whose .bin and .json exist (reference --check_existing)")
    ap.add_argument("--save-decoded-frame", "--save_decoded_frame", **flag,
                    help="with --stream-path: write the reconstruction beside the .bin (reference --save_decoded_frame)")
    ap.add_argument("--src-type", "--src_type", choices=SRC_TYPES + SRC_TYPES_422, default="yuv420",
                    help="--src is a planar 8-bit YUV 4:2:0 file (yuv420), a directory of im1.png ... / im00001.png ... (RGB), or a "
                         "raw file in one of the other formats under its ffmpeg name (10 / 12 / 16 bits, 4:4:4, NV12, P010; 4:2:2: "
                         "yuv422p .. yuv422p16le, uyvy422, yuyv422, v210)")
    ap.add_argument("--src")
    ap.add_argument("--width", type=int)
    ap.add_argument("--height", type=int)
    ap.add_argument("--frames", type=int)
    ap.add_argument("--rate-num", "--rate_num", type=int, default=4)
    ap.add_argument("--qp-i", "--qp_i", type=int, nargs="*")
    ap.add_argument("--qp-p", "--qp_p", type=int, nargs="*")
    ap.add_argument("--intra-period", type=int, default=-1)
    ap.add_argument("--reset-interval", "--reset_interval", type=int, default=32)
    _add_extension_options(ap, flag)
    ap.add_argument("--model-i", "--model_path_i", help="DMCI checkpoint (.pth.tar); synthetic weights if omitted")
    ap.add_argument("--model-p", "--model_path_p", help="DMC checkpoint")
    ap.add_argument("--force-zero-thres", "--force_zero_thres", type=float, default=0.12)
    ap.add_argument("--fp32", action="store_true")
    ap.add_argument("--bin-prefix", help="write <prefix>_q<qp>.bin")
    ap.add_argument("--out", help="JSON output path (default: stdout)")
    ap.add_argument("--verbose", type=int, default=1)
    ap.add_argument("--verbose-json", "--verbose_json", **flag, help="per-frame lists in the log (reference --verbose_json)")
    return ap


def manifest_options(args, ap):
    """(opts, gpus) of a manifest run from the parsed command line (both spellings)"""
    if not args.cuda:
        ap.error("--cuda 0: this framework has no CPU path (the reference's torch fallback is what oracle/ restates for the tests)")
    gpu_ids = args.gpu_ids or ([str(i) for i in args.cuda_idx] if args.cuda_idx else None) or visible_gpu_ids()
    gpus = args.gpus if args.gpus is not None else (len(gpu_ids) if gpu_ids else count_gpus())
    if gpu_ids and gpus > len(gpu_ids):
        ap.error("--gpus %d but only %d device ids are given / visible (%s)" % (gpus, len(gpu_ids), ",".join(gpu_ids)))
    stream_path = args.stream_path or ("out_bin" if args.write_stream else None)      # (the reference's default folder)
    opts = {k: getattr(args, k) for k in ("rate_num", "qp_i", "qp_p", "force_root_path", "force_frame_num", "force_intra_period",
                                          "reset_interval", "model_i", "model_p", "force_zero_thres", "fp32", "target_bpp",
                                          "target_kbps", "fps", "force_intra", "check_existing", "save_decoded_frame",
                                          "temporal_filter", "tf_radius", "tf_subpel", "lookahead")}
    opts.update(gpu_ids=gpu_ids, stream_path=stream_path, **crop_kwargs(vars(args)), **dup_kwargs(vars(args)),
                **deint_kwargs(vars(args)), **point_kwargs(vars(args)))
    return opts, gpus


def main(argv=None):
    ap = build_parser()
    args = ap.parse_args(argv)
    check_rate_options(args, ap)
    check_lookahead_options(args, ap)
    check_crop_options(args, ap)
    check_dup_options(args, ap)
    check_deint_options(args, ap)
    if args.test_config:
        with open(args.test_config) as f:
            config = json.load(f)
        opts, gpus = manifest_options(args, ap)
        t0 = time.time()
        log = run_config(config, opts, workers=args.worker, gpus=gpus)
        out_path = args.output_path or args.out
        if out_path:
            os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
            with open(out_path, "w") as f:
                dump_json(log, f, float_digits=6, indent=2)
        else:
            import sys
            dump_json(log, sys.stdout, float_digits=6, indent=2)
        print(f"\nTest finished: {sum(len(v) for d in log.values() for v in d.values())} points, "
              f"{(time.time() - t0) / 60:.1f} min")
        return
    if not (args.src and args.width and args.height and args.frames):
        ap.error("either --test-config or --src/--width/--height/--frames")

    res = run_sweep(lambda: load_nets(args.model_i, args.model_p, args.force_zero_thres, args.fp32, "cuda"),
                    args.src, args.width, args.height, args.frames, args.rate_num, args.qp_i or None, args.qp_p or None,
                    bin_prefix=args.bin_prefix, intra_period=args.intra_period, reset_interval=args.reset_interval,
                    src_type=args.src_type, target_bpp=target_bpp(vars(args), args.width, args.height),
                    **prefilter_kwargs(vars(args)), **lookahead_kwargs(vars(args)), **crop_kwargs(vars(args)),
                    **dup_kwargs(vars(args)), **deint_kwargs(vars(args)), **point_kwargs(vars(args)))
    text = json.dumps({str(k): v for k, v in res.items()}, indent=2)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    else:
        print(text)


if __name__ == "__main__":
    main()
