"""Repeated-frame coding (docs/frame_repeat.md; csrc/dcvc_repeat.hip): a frame that is the same picture as the frame coded
last is not pushed through the P-frame network again, the stream says "show the last picture again" in one byte
(bitstream.NalType.NAL_REPEAT).  No reference counterpart: the reference codes every frame.

RepeatDetector answers "is this model frame the picture of the last frame that was coded" with one kernel over both frames:
the largest sample difference per plane, exact, held against a tolerance on the host.  tests/repeat_ref.py restates the
kernel in numpy."""
import ctypes


def tol_fraction(tol, name="dup_tol"):
    """a tolerance in 8-bit codes -> the kernels' unit, an fp32 fraction of 255; ValueError, under the option's name, for a
    negative or NaN one.  The one conversion: harness.check_crop turns crop_tol with it too"""
    import numpy as np
    frac = float(np.float32(tol) / np.float32(255.0))
    if not frac >= 0.0:
        raise ValueError(f"{name} {tol!r}: 8-bit codes, >= 0")
    return frac


class RepeatDetector:
    """RepeatDetector(device, tol=0.0): tol in 8-bit codes (0: only a frame whose every sample equals the reference's).

    is_repeat(x, size) compares the size = (H, W) picture of the model frame x [1, 3, Hp, Wp] with the REFERENCE: the last
    frame that was no repeat - not the previous frame, so a slow ramp of steps below the tolerance can never add up to a
    jump that is not coded.  The first frame, and a frame whose size, shape or dtype differs from the reference's, is no
    repeat.  A frame is a repeat iff on all three planes the largest |x - reference| is <= tol, compared in fp32 (a NaN in
    either frame is never a repeat).  A frame that is no repeat becomes the reference.

    The detector HOLDS the reference tensor, it does not copy it: the caller must not overwrite a tensor it has passed to
    is_repeat() while it may still be the reference (until the next frame that is no repeat has been passed).

    One compare is enqueued on the current stream per call and the call waits for that compare's event only.  maxima(): the
    three maxima of the last compare as floats (None before the first compare); repeats: the frames found repeated."""

    def __init__(self, device="cuda:0", tol=0.0):
        import numpy as np
        import torch
        from . import _lib
        from .entropy import PinnedBuffer
        self.tol_codes = float(tol)
        self.tol = np.float32(tol_fraction(tol))
        self.device = torch.device(device)
        self._lib = _lib.lib()
        need = _lib.check(self._lib.dcvc_frame_maxdiff_ws_bytes(), "dcvc_frame_maxdiff_ws_bytes")
        self._ws = torch.zeros(need, dtype=torch.uint8, device=self.device)      # (zero once: every compare leaves it zero)
        self._pinned = PinnedBuffer(16)
        self._out = self._pinned.view(np.uint32, 4)
        self._event = torch.cuda.Event()
        self._ref = None             # (tensor, size) of the last frame that was no repeat
        self._maxima = None
        self.repeats = 0

    def compare(self, a, b, size):
        """the keys of the largest |a - b| per plane over the size = (H, W) picture of two model frames of one shape and
        dtype -> numpy uint32 [3]; waits for this compare's event"""
        import torch
        from . import _lib
        from . import nn as L
        a, b = L.frame(a), L.frame(b)
        if a.shape != b.shape or a.dtype != b.dtype:
            raise ValueError(f"two frames of one shape and dtype are compared, got {tuple(a.shape)} {a.dtype} and "
                             f"{tuple(b.shape)} {b.dtype}")
        st = torch.cuda.current_stream(self.device)
        code, pa, hp, wp, h, w = L.frame_args(a, size)
        _lib.check(self._lib.dcvc_frame_maxdiff(code, pa, L._p(b), hp, wp, h, w, L._p(self._ws),
                                                ctypes.c_void_p(self._pinned.ptr), ctypes.c_void_p(st.cuda_stream)),
                   "dcvc_frame_maxdiff")
        self._event.record(st)
        self._event.synchronize()
        return self._out[:3].copy()

    def is_repeat(self, x, size):
        import numpy as np
        size = (int(size[0]), int(size[1]))
        ref = self._ref
        if ref is None or ref[1] != size or ref[0].shape != x.shape or ref[0].dtype != x.dtype:
            self._ref = (x, size)
            return False
        keys = self.compare(x, ref[0], size)
        self._maxima = keys.view(np.float32)
        if bool(np.all(self._maxima <= self.tol)):       # (fp32 against fp32; a NaN fails)
            self.repeats += 1
            return True
        self._ref = (x, size)
        return False

    def maxima(self):
        return None if self._maxima is None else tuple(float(v) for v in self._maxima)
