"""Active-area coding (docs/active_area.md; csrc/dcvc_bars.hip): the black bars of letterboxed / pillarboxed material are
found on the device, the encoder codes the window between them and the decode side pastes the window back into the full
picture.  No reference counterpart: the reference codes every pixel of the container's picture.

BarDetector folds any number of frames into a per-row / per-column min / max envelope on the device (no read-back) and
reads the bars' extents off it with one synchronisation; ActiveArea.from_extents is the host policy that turns extents into
the window to code; window / paste are the two copies.  tests/bars_ref.py restates keys, envelope, rule and copies in numpy."""
import ctypes
from dataclasses import dataclass
from typing import Tuple


@dataclass(frozen=True)
class ActiveArea:
    """the height x width window at (top, left) of a full_height x full_width picture; colour: the (Y, U, V) of everything
    outside it, as the model's fp32 values (sample / max_val)"""
    full_height: int
    full_width: int
    top: int
    left: int
    height: int
    width: int
    colour: Tuple[float, float, float]

    def __post_init__(self):
        if not (self.height > 0 and self.width > 0 and self.top >= 0 and self.left >= 0 and
                self.top + self.height <= self.full_height and self.left + self.width <= self.full_width):
            raise ValueError(f"the window {self.width}x{self.height} at ({self.top}, {self.left}) is not inside the picture "
                             f"{self.full_width}x{self.full_height}")
        if self.top % 2 or self.left % 2:
            raise ValueError(f"the window's offsets ({self.top}, {self.left}) must be even (4:2:0 chroma)")
        if len(self.colour) != 3:
            raise ValueError("the colour has three components")

    @property
    def size(self):
        return self.height, self.width

    @property
    def full_size(self):
        return self.full_height, self.full_width

    @property
    def extents(self):
        """[top, bottom, left, right]: the rows / columns outside the window"""
        return [self.top, self.full_height - self.top - self.height, self.left, self.full_width - self.left - self.width]

    @staticmethod
    def from_extents(full_h, full_w, ext, min_size=64):
        """ext: what BarDetector.extents returns - None or (top, bottom, left, right, colour) -> the ActiveArea to code, or
        None where nothing is left to crop.  Pure host policy: each extent is rounded down to even (4:2:0 chroma: the window
        starts and ends on a chroma sample), and a dimension whose remainder would fall below min_size is not cropped (an
        all-bar picture has no remainder at all: None)."""
        if ext is None:
            return None
        top, bottom, left, right = (int(v) & ~1 for v in ext[:4])
        if full_h - top - bottom < min_size:
            top = bottom = 0
        if full_w - left - right < min_size:
            left = right = 0
        if not (top or bottom or left or right):
            return None
        return ActiveArea(int(full_h), int(full_w), top, left, full_h - top - bottom, full_w - left - right,
                          tuple(float(c) for c in ext[4]))

    @staticmethod
    def from_manual(full_h, full_w, extents, colour):
        """the window of hand-given extents (top, bottom, left, right), refused where it is odd or empty; all zero: None"""
        top, bottom, left, right = (int(v) for v in extents)
        if min(top, bottom, left, right) < 0 or (top | bottom | left | right) & 1:
            raise ValueError(f"crop {top}:{bottom}:{left}:{right}: even numbers >= 0")
        if not (top or bottom or left or right):
            return None
        return ActiveArea(int(full_h), int(full_w), top, left, full_h - top - bottom, full_w - left - right,
                          tuple(float(c) for c in colour))


class BarDetector:
    """Owns the envelope workspace (sized on first use per picture size) and one pinned result buffer.  reset(size), then
    scan(x, size) per frame - enqueued on the current stream, nothing is waited for - then extents(): the one
    synchronisation of the whole detection."""

    def __init__(self, device="cuda:0"):
        import numpy as np
        import torch
        from . import _lib
        from .entropy import PinnedBuffer
        self.device = torch.device(device)
        self._lib = _lib.lib()
        self._pinned = PinnedBuffer(8 * 4)
        self._out = self._pinned.view(np.int32, 8)
        self._size = None
        self._ws = None

    def reset(self, size):
        """an empty envelope for pictures of size = (H, W)"""
        import torch
        from . import _lib
        from . import nn as L
        h, w = (int(v) for v in size)
        if self._size != (h, w):
            need = _lib.check(self._lib.dcvc_bars_ws_bytes(h, w), "dcvc_bars_ws_bytes")
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
            self._size = (h, w)
        _lib.check(self._lib.dcvc_bars_reset(L._p(self._ws), h, w, L._stream(self.device)), "dcvc_bars_reset")

    def scan(self, x, size):
        """folds the size = (H, W) picture of the model frame x [1, 3, Hp, Wp] into the envelope"""
        from . import _lib
        from . import nn as L
        if self._size != tuple(int(v) for v in size):
            raise ValueError(f"scan() of a {size[1]}x{size[0]} picture: reset() was given {self._size}")
        x = L.frame(x)
        _lib.check(self._lib.dcvc_bars_scan(*L.frame_args(x, size), L._p(self._ws), L._stream(self.device)), "dcvc_bars_scan")

    def keys(self):
        """the envelope as it lies in the workspace (a device tensor of uint32 keys viewed as int32: rowmin[3][H],
        colmin[3][W], rowmax[3][H], colmax[3][W])"""
        import torch
        return self._ws.view(torch.int32)

    def extents(self, tol=0.0):
        """the bars of everything scanned since reset(): None (no edge line of the envelope is flat within tol), or
        (top, bottom, left, right, colour) - the numbers of leading / trailing bar rows / columns and the bars' (Y, U, V).
        Waits for the stream."""
        import numpy as np
        from . import _lib
        from . import nn as L
        if self._size is None:
            raise ValueError("extents() before reset()")
        st = L._stream(self.device)
        _lib.check(self._lib.dcvc_bars_extent(L._p(self._ws), *self._size, float(tol), ctypes.c_void_p(self._pinned.ptr), st),
                   "dcvc_bars_extent")
        _lib.check(self._lib.dcvc_stream_sync(st), "dcvc_stream_sync")
        out = self._out.copy()
        if not out[0]:
            return None
        return (*(int(v) for v in out[1:5]), tuple(float(c) for c in out[5:8].view(np.float32)))


def _padded(n, pad_to):
    return n + (-n) % pad_to


def _pad_ok(pad_to):
    if pad_to <= 0 or pad_to % 8:
        raise ValueError("pad_to must be a multiple of 8 (the kernels store 8 pixels at a time)")


def window(x, size, area, pad_to=16):
    """the model frame x [1, 3, Hp, Wp] with the size = area.full_size picture at its top left -> [1, 3, H', W']: the
    area's window, replicate-padded to a multiple of pad_to.  Enqueued on the current stream."""
    import torch
    from . import _lib
    from . import nn as L
    _pad_ok(pad_to)
    if tuple(int(v) for v in size) != area.full_size:
        raise ValueError(f"a {size[1]}x{size[0]} picture, the area belongs to {area.full_width}x{area.full_height}")
    x = L.frame(x)
    out = torch.empty((1, 3, _padded(area.height, pad_to), _padded(area.width, pad_to)), dtype=x.dtype, device=x.device)
    _lib.check(_lib.lib().dcvc_frame_window(*L.frame_args(x, size), area.top, area.left, L._p(out), out.shape[2], out.shape[3],
                                            area.height, area.width, L._stream(x.device)), "dcvc_frame_window")
    return out


def paste(x, area, pad_to=16):
    """the model frame x [1, 3, Hp, Wp] with the area's window at its top left -> [1, 3, H', W']: the full picture - the
    window where it belongs, the area's colour around it - replicate-padded to a multiple of pad_to.  Enqueued on the
    current stream."""
    import torch
    from . import _lib
    from . import nn as L
    _pad_ok(pad_to)
    x = L.frame(x)
    out = torch.empty((1, 3, _padded(area.full_height, pad_to), _padded(area.full_width, pad_to)), dtype=x.dtype,
                      device=x.device)
    colour = (ctypes.c_float * 3)(*area.colour)
    _lib.check(_lib.lib().dcvc_frame_paste(*L.frame_args(x, area.size), L._p(out), out.shape[2], out.shape[3], area.full_height,
                                           area.full_width, area.top, area.left, colour, L._stream(x.device)),
               "dcvc_frame_paste")
    return out
