"""The scaler of a reduced-resolution run (docs/reduced_resolution.md): the tables of a separable polyphase resampler, made
on the host in float64, and the device resampler that applies them to model frames (csrc/dcvc_resize.hip,
dcvc_resize_frame: one launch per frame for the three planes, fp16 and fp32).  No reference counterpart: the reference
codes a sequence at the size it arrives in.

The table definition is the one Pillow's Image.resize and torch's interpolate(antialias=True) use: the filter's support is
stretched by the scale when shrinking, every window is cut at the picture's border and its weights are normalised.
"""
import numpy as np

FILTERS = ("bilinear", "bicubic", "lanczos3")          # the container's filter ids (bitstream.NAL_DISPLAY) are the positions
MAX_RATIO = 8.0                                        # in either direction; lanczos3 at 8 needs 49 taps
MAX_TAPS = 64                                          # dcvc_resize_frame's limit


def _bilinear(t):
    t = np.abs(t)
    return np.where(t < 1.0, 1.0 - t, 0.0)


def _bicubic(t, a=-0.5):
    """Keys' cubic convolution kernel"""
    t = np.abs(t)
    return np.where(t < 1.0, ((a + 2.0) * t - (a + 3.0)) * t * t + 1.0,
                    np.where(t < 2.0, (((t - 5.0) * t + 8.0) * t - 4.0) * a, 0.0))


def _lanczos3(t):
    return np.where(np.abs(t) < 3.0, np.sinc(t) * np.sinc(t / 3.0), 0.0)


_KERNELS = {"bilinear": (1.0, _bilinear), "bicubic": (2.0, _bicubic), "lanczos3": (3.0, _lanczos3)}


def filter_taps(name, n_in, n_out):
    """-> (first int32 [n_out], coef float32 [n_out, K]): output sample j is sum_k coef[j, k] * in[first[j] + k].
    scale = n_in / n_out, fs = max(1, scale), support = a * fs; centre c = (j + 0.5) * scale, window
    [lo, hi) = [max(int(c - support + 0.5), 0), min(int(c + support + 0.5), n_in)), weights f((k - c + 0.5) / fs) for k in
    the window, divided by their sum in float64, then cast to float32.  K: the longest window; shorter rows end in zeros.
    n_in == n_out: every filter here interpolates (f(0) = 1, f = 0 at the other integers), so the table is written as the
    identity it is - first[j] = j, one weight 1.0 - instead of with the rounding residue of sinc at the integers (Pillow
    and torch skip the pass for an axis that keeps its size)."""
    if name not in _KERNELS:
        raise ValueError(f"filter {name!r}: one of {', '.join(FILTERS)}")
    n_in, n_out = int(n_in), int(n_out)
    if n_in < 1 or n_out < 1:
        raise ValueError(f"bad sizes {n_in} -> {n_out}")
    if n_in > MAX_RATIO * n_out or n_out > MAX_RATIO * n_in:
        raise ValueError(f"{n_in} -> {n_out}: a ratio above {MAX_RATIO:g} is not supported")
    if n_in == n_out:
        return np.arange(n_out, dtype=np.int32), np.ones((n_out, 1), np.float32)
    a, f = _KERNELS[name]
    scale = n_in / n_out
    fs = max(1.0, scale)
    support = a * fs
    rows = []
    for j in range(n_out):
        c = (j + 0.5) * scale
        lo, hi = max(int(c - support + 0.5), 0), min(int(c + support + 0.5), n_in)
        w = f((np.arange(lo, hi, dtype=np.float64) - c + 0.5) / fs)
        rows.append((lo, w / w.sum()))
    K = max(len(w) for _, w in rows)
    first = np.asarray([lo for lo, _ in rows], np.int32)
    coef = np.zeros((n_out, K), np.float32)
    for j, (_, w) in enumerate(rows):
        coef[j, :len(w)] = w.astype(np.float32)
    return first, coef


def padded(n, pad_to):
    return n + (-n) % pad_to


class Resampler:
    """Resamples model frames on `device`.  The tables of a (n_in, n_out, filter) are made once and stay on the device."""

    def __init__(self, device):
        import torch
        self.device = torch.device(device)
        self._tables = {}

    def tables(self, n_in, n_out, filter):
        """(first, coef, K) on the device"""
        key = (int(n_in), int(n_out), filter)
        t = self._tables.get(key)
        if t is None:
            import torch
            first, coef = filter_taps(filter, n_in, n_out)
            t = self._tables[key] = (torch.from_numpy(first).to(self.device), torch.from_numpy(coef).to(self.device),
                                     coef.shape[1])
        return t

    def resample(self, x, size_in, size_out, filter="lanczos3", pad_to=16):
        """x [1, 3, Hp, Wp] (fp16 / fp32) with the valid region size_in = (H, W) at its top left -> [1, 3, HO', WO']: the
        size_out = (HO, WO) picture, replicate-padded to a multiple of pad_to.  Enqueued on the current stream, nothing is
        waited for.  size_in == size_out: x itself, nothing is launched."""
        import torch
        from . import _lib
        from . import nn as L
        (H, W), (HO, WO) = (int(v) for v in size_in), (int(v) for v in size_out)
        if filter not in FILTERS:
            raise ValueError(f"filter {filter!r}: one of {', '.join(FILTERS)}")
        if (H, W) == (HO, WO):
            return x
        x = L.frame(x)
        first_h, coef_h, kh = self.tables(W, WO, filter)
        first_v, coef_v, kv = self.tables(H, HO, filter)
        out = torch.empty((1, 3, padded(HO, pad_to), padded(WO, pad_to)), dtype=x.dtype, device=x.device)
        _lib.check(_lib.lib().dcvc_resize_frame(*L.frame_args(x, (H, W)), L._p(out), out.shape[2], out.shape[3], HO, WO,
                                                L._p(first_h), L._p(coef_h), kh, L._p(first_v), L._p(coef_v), kv, L._stream()),
                   "dcvc_resize_frame")
        return out


def parse_size(text):
    """'WxH' (the spelling of --coded-size) -> (height, width)"""
    parts = str(text).lower().split("x")
    if len(parts) != 2 or not all(p.isdigit() for p in parts):
        raise ValueError(f"size {text!r}: WIDTHxHEIGHT, e.g. 1280x720")
    return int(parts[1]), int(parts[0])


def check_coded_size(coded_size, height, width):
    """the coded size of a height x width source: None (no scaling: absent, or equal to the source), or (ch, cw) with
    16 <= ch <= height and 16 <= cw <= width"""
    if coded_size is None:
        return None
    ch, cw = (int(v) for v in coded_size)
    if ch < 16 or cw < 16:
        raise ValueError(f"coded size {cw}x{ch}: at least 16 in each dimension")
    if ch > height or cw > width:
        raise ValueError(f"coded size {cw}x{ch} above the source's {width}x{height}")
    if height > MAX_RATIO * ch or width > MAX_RATIO * cw:
        raise ValueError(f"coded size {cw}x{ch}: more than {MAX_RATIO:g} times below the source's {width}x{height}")
    return None if (ch, cw) == (height, width) else (ch, cw)
