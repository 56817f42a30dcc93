"""PSNR and MS-SSIM of decoded frames on the device (csrc/dcvc_metrics.hip): what harness.yuv420_distortion /
yuv420_msssim / rgb_distortion compute with torch glue and host numpy / scipy, as HIP kernels - the planes the
reference's get_distortion compares (test_video.py:94-127), their squared error and the per-scale SSIM / contrast
means of calc_msssim (src/utils/metrics.py:9-68) in fp64, written by the kernels into pinned host memory.  Everything
of a frame is enqueued on the current stream, then the stream is synchronised ONCE; no torch kernel runs and no plane
is copied to the host."""
import ctypes

import numpy as np
import torch

from . import _lib
from . import nn as L
from .entropy import PinnedBuffer
from .harness import _MSSSIM_WEIGHTS, psnr_from_mse, source_planes

# (16-bit samples travel as torch.uint16 or as an int16 view of the same words: the kernels read them unsigned)
_TYPE = {torch.float16: _lib.F16, torch.float32: _lib.F32, torch.uint8: _lib.U8, torch.uint16: _lib.U16, torch.int16: _lib.U16}
_SLOT = 1 + 2 * 5          # doubles per measured plane pair: the squared error, then (ssim mean, cs mean) per level
_SLOTS = 4                 # Y, U, V / R, G, B and the whole RGB picture


def msssim_from_stats(ssim_mean, cs_mean):
    """the last line of calc_msssim (metrics.py:67-68) from the per-level means; a negative contrast mean to a
    fractional power is NaN, as in the reference"""
    levels = len(ssim_mean)
    weights = np.asarray(_MSSSIM_WEIGHTS[levels])
    cs_mean, ssim_mean = np.asarray(cs_mean, np.float64), np.asarray(ssim_mean, np.float64)
    with np.errstate(invalid="ignore"):
        return float(np.prod(cs_mean[:levels - 1] ** weights[:levels - 1]) * ssim_mean[levels - 1] ** weights[levels - 1])


def _type_code(t):
    try:
        return _TYPE[t.dtype]
    except KeyError:
        raise _lib.DcvcError(f"unsupported plane dtype {t.dtype}: the metric kernels read uint8, uint16, float16 or float32") from None


class DeviceMetrics:
    """Owns the reconstruction-plane buffers, the MS-SSIM workspace and the pinned result buffer; sized on first use per
    (H, W, dtype) and reused: no allocation per frame.  One instance serves one stream at a time."""

    def __init__(self, device="cuda:0"):
        self.device = torch.device(device)
        self._lib = _lib.lib()
        self._planes = {}                                   # (kind, H, W, dtype) -> reconstruction plane tensors
        self._ws, self._ws_bytes = None, 0                  # MS-SSIM workspace (the largest plane seen)
        self._sse_ws = torch.empty(_lib.SSE_BLOCKS, dtype=torch.float64, device=self.device)
        self._pinned = PinnedBuffer(8 * _SLOT * _SLOTS)
        self._out = self._pinned.view(np.float64, _SLOT * _SLOTS)

    # ------------------------------------------------------------------------------------------ enqueue
    def _stream(self):
        return L._stream(self.device)

    def _slot_ptr(self, slot, offset=0):
        return ctypes.c_void_p(self._pinned.ptr + 8 * (slot * _SLOT + offset))

    def _workspace(self, h, w):
        need = _lib.check(self._lib.dcvc_msssim_ws_bytes(h, w), "dcvc_msssim_ws_bytes")
        if need > self._ws_bytes:
            self._ws, self._ws_bytes = torch.empty(need, dtype=torch.uint8, device=self.device), need
        return self._ws

    def _enqueue_sse(self, slot, a, ta, b, tb, n, stream):
        _lib.check(self._lib.dcvc_sse(ta, a, tb, b, n, L._p(self._sse_ws), self._slot_ptr(slot), stream), "dcvc_sse")

    def _enqueue_msssim(self, slot, a, ta, b, tb, h, w, data_range, stream):
        """-> levels"""
        if h < 88 or w < 88:
            raise ValueError("MS-SSIM needs planes of at least 88 x 88 (the reference asserts)")
        levels = ctypes.c_int(0)
        _lib.check(self._lib.dcvc_msssim_stats(ta, a, tb, b, h, w, float(data_range), L._p(self._workspace(h, w)),
                                               self._slot_ptr(slot, 1), ctypes.byref(levels), stream), "dcvc_msssim_stats")
        return levels.value

    def _sync(self, stream):
        _lib.check(self._lib.dcvc_stream_sync(stream), "dcvc_stream_sync")

    def _stats(self, slot, levels):
        o = self._out[slot * _SLOT + 1: slot * _SLOT + 1 + 2 * levels]
        return o[0::2].copy(), o[1::2].copy()

    @staticmethod
    def _check_pair(a, b):
        if a.shape != b.shape or not (a.is_contiguous() and b.is_contiguous()):
            raise ValueError("the metric kernels compare two contiguous tensors of one shape")

    # ------------------------------------------------------------------------------------------ single planes
    def sse(self, a, b):
        """sum((a - b)^2) in float64 of two device tensors (uint8 / float16 / float32, same shape)"""
        self._check_pair(a, b)
        st = self._stream()
        self._enqueue_sse(0, L._p(a), _type_code(a), L._p(b), _type_code(b), a.numel(), st)
        self._sync(st)
        return float(self._out[0])

    def msssim_stats(self, a, b, data_range=255):
        """(ssim mean per level, cs mean per level) of two [H, W] device planes"""
        self._check_pair(a, b)
        h, w = a.shape
        st = self._stream()
        levels = self._enqueue_msssim(0, L._p(a), _type_code(a), L._p(b), _type_code(b), h, w, data_range, st)
        self._sync(st)
        return self._stats(0, levels)

    def msssim(self, a, b, data_range=255):
        """harness.calc_msssim of two [H, W] device planes"""
        return msssim_from_stats(*self.msssim_stats(a, b, data_range))

    # ------------------------------------------------------------------------------------------ frames
    def yuv420_planes(self, x_hat, height, width):
        """decoded [1,3,H',W'] -> the planes the metrics compare: clamp(x * 255, 0, 255), chroma = 2x2 mean, NOT rounded,
        in x_hat's dtype (enqueued on the current stream; the returned tensors are this object's buffers, overwritten
        by the next call at the same size)"""
        if not x_hat.is_contiguous():
            raise ValueError("x_hat must be contiguous")
        key = ("yuv", height, width, x_hat.dtype)
        planes = self._planes.get(key)
        if planes is None:
            planes = self._planes[key] = (torch.empty((height, width), dtype=x_hat.dtype, device=self.device),
                                          torch.empty((height // 2, width // 2), dtype=x_hat.dtype, device=self.device),
                                          torch.empty((height // 2, width // 2), dtype=x_hat.dtype, device=self.device))
        _lib.check(self._lib.dcvc_frame_to_yuv420_planes(*L.frame_args(x_hat, (height, width)), L._p(planes[0]), L._p(planes[1]),
                                                         L._p(planes[2]), self._stream()), "dcvc_frame_to_yuv420_planes")
        return planes

    def yuv420(self, x_hat, y, u, v, calc_ssim=False):
        """harness.yuv420_distortion and yuv420_msssim: x_hat [1,3,H',W'] (model dtype), y/u/v uint8 device planes ->
        (psnr, msssim), each [(6 Y + U + V) / 8, Y, U, V]; msssim zeros without calc_ssim"""
        H, W = y.shape
        st = self._stream()
        rec = self.yuv420_planes(x_hat, H, W)
        tr, levels = L.dtype_code(x_hat.dtype), [0, 0, 0]
        for k, (src, r) in enumerate(zip((y, u, v), rec)):
            self._check_pair(src, r)
            self._enqueue_sse(k, L._p(src), _type_code(src), L._p(r), tr, r.numel(), st)
            if calc_ssim:
                levels[k] = self._enqueue_msssim(k, L._p(src), _type_code(src), L._p(r), tr, r.shape[0], r.shape[1], 255, st)
        self._sync(st)
        psnr = [psnr_from_mse(float(self._out[k * _SLOT]) / rec[k].numel()) for k in range(3)]
        ms = [msssim_from_stats(*self._stats(k, levels[k])) for k in range(3)] if calc_ssim else [0.0, 0.0, 0.0]
        comb = lambda m: [(6 * m[0] + m[1] + m[2]) / 8] + m
        return comb(psnr), comb(ms)

    def metric_planes(self, x_hat, height, width, fmt):
        """decoded [1,3,H',W'] -> the fp32 planes the metrics of a PixelFormat source compare: clip(., 0, 1) * max_val,
        4:2:0 chroma = the fp32 2x2 mean, NOT rounded - fp32 whatever x_hat's dtype (fp16 cannot hold a 10-bit value with
        sub-LSB precision).  Enqueued on the current stream; the tensors are this object's buffers."""
        if not x_hat.is_contiguous():
            raise ValueError("x_hat must be contiguous")
        key = ("pix", height, width, fmt.chroma)
        planes = self._planes.get(key)
        if planes is None:
            ch, cw = {444: (height, width), 422: (height, width // 2)}.get(fmt.chroma, (height // 2, width // 2))
            planes = self._planes[key] = (torch.empty((height, width), dtype=torch.float32, device=self.device),
                                          torch.empty((ch, cw), dtype=torch.float32, device=self.device),
                                          torch.empty((ch, cw), dtype=torch.float32, device=self.device))
        code, *frame = L.frame_args(x_hat, (height, width))
        _lib.check(self._lib.dcvc_frame_to_metric_planes(code, fmt.chroma, fmt.max_val, *frame, L._p(planes[0]), L._p(planes[1]),
                                                         L._p(planes[2]), self._stream()), "dcvc_frame_to_metric_planes")
        return planes

    def yuv(self, x_hat, planes, fmt, calc_ssim=False, width=None):
        """harness.pixfmt_distortion on the device: x_hat [1,3,H',W'] (model dtype), planes: the source's device planes as
        its reader delivers them (uint8 / uint16; the chroma of NV12 / P010 is de-interleaved and P010's words are
        shifted down here by harness.source_planes, torch glue on the measuring side) -> (psnr, msssim), each
        [(6 Y + U + V) / 8, Y, U, V] with data_range = max_val; msssim zeros without calc_ssim"""
        y, u, v = source_planes(planes, fmt, width)     # (width: the picture's, for a packed 4:2:2 surface)
        H, W = y.shape
        st = self._stream()
        rec = self.metric_planes(x_hat, H, W, fmt)
        levels = [0, 0, 0]
        for k, (src, r) in enumerate(zip((y, u, v), rec)):
            self._check_pair(src, r)
            self._enqueue_sse(k, L._p(src), _type_code(src), L._p(r), _lib.F32, r.numel(), st)
            if calc_ssim:
                levels[k] = self._enqueue_msssim(k, L._p(src), _type_code(src), L._p(r), _lib.F32, r.shape[0], r.shape[1],
                                                 fmt.max_val, st)
        self._sync(st)
        psnr = [psnr_from_mse(float(self._out[k * _SLOT]) / rec[k].numel(), float(fmt.max_val)) for k in range(3)]
        ms = [msssim_from_stats(*self._stats(k, levels[k])) for k in range(3)] if calc_ssim else [0.0, 0.0, 0.0]
        comb = lambda m: [(6 * m[0] + m[1] + m[2]) / 8] + m
        return comb(psnr), comb(ms)

    def rgb(self, x_hat, rgb, calc_ssim=False):
        """harness.rgb_distortion: x_hat [1,3,H',W'] YCbCr (model dtype), rgb uint8 [3,H,W] (device) -> ([psnr], [msssim]):
        PSNR over the whole picture, MS-SSIM the mean over the three planes"""
        if not x_hat.is_contiguous():
            raise ValueError("x_hat must be contiguous")
        _, H, W = rgb.shape
        key = ("rgb", H, W, x_hat.dtype)
        rec = self._planes.get(key)
        if rec is None:
            rec = self._planes[key] = torch.empty((3, H, W), dtype=x_hat.dtype, device=self.device)
        self._check_pair(rgb, rec)
        st = self._stream()
        tr, ts = L.dtype_code(x_hat.dtype), _type_code(rgb)
        _lib.check(self._lib.dcvc_frame_to_rgb(*L.frame_args(x_hat, (H, W)), L._p(rec), st), "dcvc_frame_to_rgb")
        self._enqueue_sse(3, L._p(rgb), ts, L._p(rec), tr, 3 * H * W, st)
        levels = 0
        if calc_ssim:
            for k in range(3):
                levels = self._enqueue_msssim(k, ctypes.c_void_p(rgb.data_ptr() + k * H * W * rgb.element_size()), ts,
                                              ctypes.c_void_p(rec.data_ptr() + k * H * W * rec.element_size()), tr, H, W, 255, st)
        self._sync(st)
        psnr = psnr_from_mse(float(self._out[3 * _SLOT]) / (3 * H * W))
        ms = sum(msssim_from_stats(*self._stats(k, levels)) for k in range(3)) / 3 if calc_ssim else 0.0
        return [psnr], [ms]
