"""Frame analysis for the encoder's scene-cut decision (csrc/dcvc_analysis.hip; no reference counterpart: the reference
harness places I frames by fi % intra_period only).  The luma plane of the model input is read where it lies and reduced
to a low-resolution plane of 8 x 8 block sums of 10-bit samples; from it and the previous frame's plane the kernels form
three integers - inter = sum |L - L_prev|, intra = sum of the smaller of the differences to the left and the top
neighbour, total = sum L - and write them into pinned host memory.  Integer arithmetic after the per-sample quantisation:
the figures do not depend on reduction order (tests/analysis_ref.py restates them in numpy, bit for bit).

The analysis runs on a HIP stream of its own behind an event, and only that stream is synchronised: kernels the caller
has in flight on the encode stream (SequenceEncoder(defer_stream=True): the previous frame's back half) keep running.
FrameStats is also the complexity measure a rate controller would start from."""
import ctypes
from typing import NamedTuple


class FrameStats(NamedTuple):
    inter: int          # sum |L - L_prev| over the 8 x 8 blocks (0 without a previous plane)
    intra: int          # sum min(|L - left|, |L - top|)
    total: int          # sum L
    blocks: int         # number of 8 x 8 blocks
    has_prev: bool      # a previous plane was compared


def is_cut(stats, scenecut):
    """the frame differs from its predecessor at least scenecut percent as much as it differs from itself one block
    over (Python integers: nothing overflows)"""
    return bool(stats.has_prev and 100 * int(stats.inter) >= int(scenecut) * max(int(stats.intra), 1))


class FrameAnalyzer:
    """Owns two ping-pong low-resolution planes, the workspace, one pinned result buffer and a HIP stream; sized on first
    use per (H, W) and reused: no allocation per frame.  One instance follows one sequence."""

    def __init__(self, device="cuda:0"):
        import numpy as np
        import torch
        from . import _lib
        from .entropy import PinnedBuffer
        self.device = torch.device(device)
        self._lib = _lib.lib()
        self.stream = torch.cuda.Stream(self.device)
        self._ready = torch.cuda.Event()          # recorded per call when the caller passes no event of its own
        self._pinned = PinnedBuffer(4 * 8)
        self._out = self._pinned.view(np.uint64, 4)
        self._size = None
        self._planes = self._ws = None
        self._cur = 0                 # index of the plane the NEXT call writes
        self._has_prev = False

    def reset(self):
        """forget the previous plane: the next frame is analysed as the first of a sequence"""
        self._has_prev = False

    def _buffers(self, h, w):
        import torch
        from . import _lib
        if self._size != (h, w):
            need = _lib.check(self._lib.dcvc_frame_analysis_ws_bytes(h, w), "dcvc_frame_analysis_ws_bytes")
            self._planes = [torch.empty((h // 8, w // 8), dtype=torch.uint16, device=self.device) for _ in range(2)]
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
            self._size, self._has_prev = (h, w), False
        return self._planes, self._ws

    def analyze(self, x, ready=None):
        """x: the [1, 3, Hp, Wp] model input (fp16 / fp32; plane 0 is the luma, read in place).  ready: a
        torch.cuda.Event recorded where x became ready (a loader stream, or the encode stream before the previous frame
        was enqueued); without it one is recorded on the current stream at the call.  -> FrameStats"""
        import torch
        from . import _lib
        from . import nn as L
        if x.dim() != 4 or x.shape[0] != 1 or x.stride(3) != 1:
            raise ValueError("analyze() takes the [1, C, H, W] model input with unit column stride")
        h, w = int(x.shape[2]), int(x.shape[3])
        planes, ws = self._buffers(h, w)
        if ready is None:
            ready = self._ready                   # (free again: the last call waited for its stream)
            ready.record(torch.cuda.current_stream(self.device))
        self.stream.wait_event(ready)
        cur, prev = planes[self._cur], planes[self._cur ^ 1]
        st = ctypes.c_void_p(self.stream.cuda_stream)
        _lib.check(self._lib.dcvc_frame_analyze(L.dtype_code(x.dtype), L._p(x), int(x.stride(2)), h, w,
                                                L._p(prev) if self._has_prev else None, L._p(cur), L._p(ws),
                                                ctypes.c_void_p(self._pinned.ptr), st), "dcvc_frame_analyze")
        _lib.check(self._lib.dcvc_stream_sync(st), "dcvc_stream_sync")
        stats = FrameStats(int(self._out[0]), int(self._out[1]), int(self._out[2]), int(self._out[3]), self._has_prev)
        self._cur ^= 1
        self._has_prev = True
        return stats
