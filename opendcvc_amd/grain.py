"""Film-grain synthesis (docs/film_grain.md, csrc/dcvc_grain.hip; no reference counterpart): the parameters a grain unit of
the stream carries (bitstream.NalType.NAL_GRAIN), the device side that puts grain on decoded pictures (dcvc_grain_apply: one
launch per frame for the three planes, fp16 and fp32) and measures it (dcvc_grain_stats: an integer table, one read-back), and
the host code that turns the table into parameters.  The model is stateless and integer: the kernel and the numpy restatement
tests/grain_ref.py agree bit for bit."""
import ctypes
import math
from dataclasses import dataclass
from typing import Optional, Tuple

TAPS = ((1,), (1, 2, 1), (1, 4, 6, 4, 1))              # the shapes' 1-D binomials (corr 0, 1, 2)
VAR_WHITE = 21845                                      # 4 * (256^2 - 1) / 12: four bytes summed
GAIN = (3547, 591, 51)                                 # round(2^19 / sqrt(VAR_WHITE * (sum of taps^2)^2))
UNIT_BODY_BYTES = 13
MIN_BLOCKS = 4                                         # flat blocks a line of the table needs to count
TABLE_LINES = 12                                       # 8 bands, Cb, Cr, lag-1 horizontal, lag-1 vertical: (count, sum) each
BLOCK = 16


def _autocorr(taps):
    n = len(taps)
    e = sum(a * a for a in taps)
    return [sum(taps[i] * taps[i + d] for i in range(n - d)) / e for d in range(n)]


# std of g * gain over the common unit 2^19; the lag-1 correlation of each shape; the share of a shaped field's variance that
# the mean of a 16 x 16 block carries (all from the taps, docs/film_grain.md)
GAIN_RATIO = tuple(g * math.sqrt(VAR_WHITE) * sum(a * a for a in t) / 2.0 ** 19 for g, t in zip(GAIN, TAPS))
LAG1 = tuple((_autocorr(t) + [0.0])[1] for t in TAPS)
CORR_THRESHOLDS = ((LAG1[0] + LAG1[1]) / 2, (LAG1[1] + LAG1[2]) / 2)
BLOCK_MEAN_SHARE = tuple((sum((_autocorr(t)[abs(i - j)] if abs(i - j) < len(t) else 0.0)
                              for i in range(BLOCK) for j in range(BLOCK)) / BLOCK ** 2) ** 2 for t in TAPS)


@dataclass(frozen=True)
class GrainParams:
    """seed 0 .. 65535; corr 0, 1, 2 (grain size); scale_y: luma strength at eight intensity bands, scale_cb / scale_cr: the
    chroma planes' - standard deviations in units of 2^-11 of full scale, 0 .. 255.  All strengths 0: no grain."""
    seed: int = 0
    corr: int = 0
    scale_y: Tuple[int, ...] = (0,) * 8
    scale_cb: int = 0
    scale_cr: int = 0

    def __post_init__(self):
        object.__setattr__(self, "scale_y", tuple(int(v) for v in self.scale_y))
        for name in ("seed", "corr", "scale_cb", "scale_cr"):
            object.__setattr__(self, name, int(getattr(self, name)))
        if not 0 <= self.seed < 1 << 16:
            raise ValueError(f"grain seed {self.seed} is not a 16-bit word")
        if self.corr not in (0, 1, 2):
            raise ValueError(f"grain corr {self.corr}: 0, 1 or 2")
        if len(self.scale_y) != 8:
            raise ValueError(f"grain scale_y has {len(self.scale_y)} values, not 8")
        if not all(0 <= v < 256 for v in self.scale_y + (self.scale_cb, self.scale_cr)):
            raise ValueError("a grain strength is outside 0 .. 255")

    @property
    def active(self):
        return any(self.scale_y) or self.scale_cb > 0 or self.scale_cr > 0

    def to_bytes(self):
        """the 13-byte body of a grain unit"""
        return self.seed.to_bytes(2, "little") + bytes((self.corr,) + self.scale_y + (self.scale_cb, self.scale_cr))

    @staticmethod
    def from_bytes(data):
        if len(data) != UNIT_BODY_BYTES:
            raise ValueError(f"a grain unit's body has {UNIT_BODY_BYTES} bytes, got {len(data)}")
        return GrainParams(int.from_bytes(data[:2], "little"), data[2], tuple(data[3:11]), data[11], data[12])


def _c_params(p):
    from ._lib import GrainParamsC
    return GrainParamsC(p.seed, p.corr, (ctypes.c_uint8 * 8)(*p.scale_y), p.scale_cb, p.scale_cr)


def params_from_stats(table, seed) -> Optional[GrainParams]:
    """the table of dcvc_grain_stats ([12][2] integers: (count, sum) per line) -> GrainParams, or None where no band has
    MIN_BLOCKS flat blocks or every strength rounds to 0.  Pure host code (docs/film_grain.md, "Estimation")."""
    t = [(int(row[0]), int(row[1])) for row in table]
    if len(t) != TABLE_LINES:
        raise ValueError(f"a grain table has {TABLE_LINES} lines, got {len(t)}")
    v_y = sum(s for _, s in t[:8])
    rho = (t[10][1] + t[11][1]) / (2.0 * 240.0 * v_y) if v_y > 0 else 0.0
    corr = 0 if rho < CORR_THRESHOLDS[0] else 1 if rho < CORR_THRESHOLDS[1] else 2

    def strength(count, total):
        var = max(total, 0) / (count * 65536.0 * (1.0 - BLOCK_MEAN_SHARE[corr]))
        return min(int(math.floor(math.sqrt(var) / 2.0 / GAIN_RATIO[corr] + 0.5)), 255)

    populated = [k for k in range(8) if t[k][0] >= MIN_BLOCKS]
    if not populated:
        return None
    own = {k: strength(*t[k]) for k in populated}
    scale_y = tuple(own[min(populated, key=lambda j: (abs(j - k), j))] for k in range(8))
    cb, cr = (strength(*t[line]) if t[line][0] >= MIN_BLOCKS else 0 for line in (8, 9))
    p = GrainParams(int(seed) & 0xFFFF, corr, scale_y, cb, cr)
    return p if p.active else None


class FilmGrain:
    """Grain on model frames [1, 3, Hp, Wp] on `device`.  Owns the 192-byte table of the estimator; nothing else is
    allocated, and apply() waits for nothing."""

    def __init__(self, device="cuda:0"):
        import torch
        self.device = torch.device(device)
        self._table = torch.zeros((TABLE_LINES, 2), dtype=torch.int64, device=self.device)

    def apply(self, x, size, params, t, out=None):
        """x with the grain of `params` for frame counter t on its size = (H, W) picture; elements outside it are copied.
        out: None (a new tensor) or a contiguous tensor like x, x itself included.  Enqueued on the current stream."""
        import torch
        from . import _lib
        from . import nn as L
        x = L.frame(x)
        if out is None:
            out = torch.empty_like(x)
        elif out.shape != x.shape or out.dtype != x.dtype or not out.is_contiguous():
            raise ValueError("out must be a contiguous tensor of x's shape and type")
        _lib.check(_lib.lib().dcvc_grain_apply(*L.frame_args(x, size), L._p(out), _c_params(params), int(t) & 0xFFFFFFFF,
                                               L._stream()), "dcvc_grain_apply")
        return out

    def stats(self, noisy, clean, size):
        """the table of every whole flat 16 x 16 block of the size = (H, W) picture: int64 numpy [12, 2], one read-back"""
        from . import _lib
        from . import nn as L
        noisy, clean = L.frame(noisy), L.frame(clean)
        if noisy.shape != clean.shape or noisy.dtype != clean.dtype:
            raise ValueError("noisy and clean must have one shape and type")
        code, _, Hp, Wp, H, W = L.frame_args(clean, size)
        _lib.check(_lib.lib().dcvc_grain_stats(code, L._p(noisy), L._p(clean), Hp, Wp, H, W, L._p(self._table), L._stream()),
                   "dcvc_grain_stats")
        return self._table.cpu().numpy()

    def estimate(self, noisy, clean, size, seed):
        return params_from_stats(self.stats(noisy, clean, size), seed)
