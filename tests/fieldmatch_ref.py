"""numpy restatement of the deinterlacer's film mode (docs/deinterlace.md, "Film mode"; csrc/dcvc_fieldmatch.hip): the comb
measure of the two candidate fields, the rule, the weave and the stateful object - integer and exact, so the kernels are held
against it bit for bit (tests/test_gpu_fieldmatch.py).  The filter of a frame that matches nothing is deint_ref's."""
import numpy as np

import deint_ref as R

T = 36                             # a difference of 9 eight-bit codes, in 10-bit codes
MI = 20                            # combed samples a 16 x 16 block may hold
BLOCK = 16


def comb_max(cur_q, other_q, H, W, parity):
    """the largest number of combed samples in one 16 x 16 block: the kept field is cur_q's, the other field other_q's
    (quantised luma [H, W]) -> python int"""
    rows = np.asarray([y for y in range(2, H - 2) if y % 2 != parity], dtype=np.int64)
    if not rows.size:
        return 0
    a, b, s, d, e = other_q[rows - 2], cur_q[rows - 1], other_q[rows], cur_q[rows + 1], other_q[rows + 2]
    d1, d2 = s - b, s - d
    combed = (((d1 > T) & (d2 > T)) | ((d1 < -T) & (d2 < -T))) & (np.abs(a + 4 * s + e - 3 * (b + d)) > 6 * T)
    counts = np.zeros(((H + BLOCK - 1) // BLOCK, (W + BLOCK - 1) // BLOCK), np.int64)
    np.add.at(counts, (rows[:, None] // BLOCK, np.arange(W)[None, :] // BLOCK), combed)
    return int(counts.max())


def field_match(cur, prev, H, W, parity):
    """cur / prev [3, Hp, Wp] (prev None: no previous frame) -> (max_c, max_p, filter, weave); max_p is 0 without prev"""
    q = R.quant(cur[0, :H, :W])
    max_c = comb_max(q, q, H, W, parity)
    max_p = comb_max(q, R.quant(prev[0, :H, :W]), H, W, parity) if prev is not None else 0
    if max_c <= MI:
        return max_c, max_p, 0, 0
    if prev is not None and max_p <= MI:
        return max_c, max_p, 0, 1
    return max_c, max_p, 1, 0


def field_weave(out, prev, H, W, parity, chroma_lines, weave):
    """out / prev [3, Hp, Wp] -> a new out.  weave 0: out as it is.  Else every row of the picture that is not kept takes
    prev's W samples, bit for bit, and out's replicate pad follows: to the right of those rows, and below the picture where
    its last row is one of them"""
    out = np.array(out)
    if not weave:
        return out
    Hp, Wp = out.shape[-2:]
    for p in range(3):
        L = 1 if p == 0 else chroma_lines
        for y in R.missing_rows(H, parity, L):
            out[p, y, :W] = prev[p, y, :W]
            out[p, y, W:] = prev[p, y, W - 1]
        if ((H - 1) // L) % 2 != parity:
            out[p, H:] = out[p, H - 1]
    return out


class Deinterlacer:
    """opendcvc_amd.deinterlace.Deinterlacer in mode "film" on numpy frames [3, Hp, Wp]"""

    def __init__(self, order="tff", chroma_lines=1):
        assert order in ("tff", "bff")
        self.parity, self.chroma_lines = 0 if order == "tff" else 1, chroma_lines
        self.judged = self.passed = self.woven = self.filtered = 0
        self.maxima = []                                   # (max_c, max_p) of every frame
        self.prev = None

    def reset(self):
        self.prev = None

    def filter(self, x, size):
        H, W = size
        R.check_size(H, self.chroma_lines)
        prev = self.prev
        if prev is not None and (prev[1] != (H, W) or prev[0].shape != x.shape or prev[0].dtype != x.dtype):
            prev = None
        p = None if prev is None else prev[0]
        max_c, max_p, filt, weave = field_match(x, p, H, W, self.parity)
        self.maxima.append((max_c, max_p))
        self.judged += 1
        self.filtered += filt
        self.woven += weave
        self.passed += 1 - filt - weave
        self.prev = (x, (H, W))
        out = R.deinterlace(x, p, H, W, self.parity, self.chroma_lines, filt)
        return out if p is None else field_weave(out, p, H, W, self.parity, self.chroma_lines, weave)

    def matches(self):
        return self.passed, self.woven, self.filtered

    def counts(self):
        return self.judged, self.filtered


def _weave_plane(first, second, parity):
    out = np.array(first)
    rows = np.arange(out.shape[0]) % 2 != parity
    out[rows] = second[rows]
    return out


def telecine(film_frames, pattern, parity=0):
    """film_frames: deint_ref.make_clip's frames - [3, H, W] (4:4:4) or (y, u, v) planes (4:2:0) - of a progressive clip;
    pattern: per output frame (the film frame of the field that comes first, the film frame of the other field) -> the frames of
    a telecined clip in the same form.  Every plane is woven by field in ITS OWN rows (in 4:2:0 the chroma rows alternate
    between the fields); parity: the rows of the first field"""
    out = []
    for i, j in pattern:
        a, b = film_frames[i], film_frames[j]
        if isinstance(a, tuple):
            out.append(tuple(_weave_plane(pa, pb, parity) for pa, pb in zip(a, b)))
        else:
            out.append(np.stack([_weave_plane(pa, pb, parity) for pa, pb in zip(a, b)]))
    return out


PULLDOWN = ((0, 0), (0, 1), (1, 2), (2, 2), (3, 3), (4, 4), (4, 5))
