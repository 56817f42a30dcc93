"""Placement helpers of tests/test_gpu_frame_io_placement.py: guarded device buffers, sources with junk around them, the
case tables (pictures, pitches, base offsets) of the streaming frame I/O kernels of csrc/dcvc_pixfmt.hip and the test's own
restatement of their access-class rule, so that the tables can assert on the CPU which classes they reach."""
import numpy as np

import pixfmt_ref as R

F = np.float32
GUARD = 64                       # least number of canary bytes in front of and behind a region
FILLS = (0xA5, 0x3C)             # two canaries: a stray store cannot write both values

# name: (chroma, bit depth, semi_planar, msb_aligned)
FORMATS = {"yuv420p": (420, 8, 0, 0), "yuv420p10le": (420, 10, 0, 0), "yuv420p16le": (420, 16, 0, 0), "nv12": (420, 8, 1, 0),
           "p010le": (420, 10, 1, 1), "yuv444p": (444, 8, 0, 0), "yuv444p12le": (444, 12, 0, 0)}
# widths below one 8-pixel piece, W % 8 in {0, 2, 4, 6} and odd widths, one chroma row, more than one piece per row
PICTURES = {420: [(2, 2), (2, 6), (4, 12), (6, 10), (8, 16), (10, 22), (18, 40)],
            444: [(1, 1), (3, 5), (5, 9), (2, 12), (7, 17), (9, 24)]}
# (luma pitch extra, chroma pitch extra, luma offset, u / uv offset, v offset), all in samples
PLANAR_PLACEMENTS = [(0, 0, 0, 0, 0), (8, 4, 0, 0, 0), (8, 4, 8, 8, 8), (8, 4, 4, 4, 4), (8, 4, 0, 2, 0), (4, 2, 0, 0, 0),
                     (4, 2, 4, 2, 2), (2, 2, 0, 0, 0), (2, 2, 2, 1, 1), (1, 1, 0, 0, 0), (1, 1, 1, 1, 1), (8, 4, 1, 0, 0),
                     (8, 4, 0, 0, 1), (0, 0, 8, 4, 2), (8, 8, 8, 8, 8)]
# an interleaved row: even pitch extras and offsets that keep a (U, V) pair aligned (the entry refuses the others); the
# pitch (8, 8) is added so that a pitched interleaved row can keep the widest class (W + 4 is no multiple of 8 where W is)
SEMI_PLACEMENTS = [(0, 0, 0, 0, 0), (8, 8, 0, 0, 0), (8, 8, 8, 8, 0), (8, 4, 0, 0, 0), (8, 8, 4, 4, 0), (8, 8, 0, 4, 0),
                   (4, 2, 0, 0, 0), (4, 2, 4, 2, 0), (2, 2, 0, 0, 0), (2, 2, 2, 2, 0), (1, 2, 0, 0, 0), (1, 2, 1, 2, 0),
                   (8, 8, 1, 0, 0), (8, 8, 0, 2, 0)]


def layout_of(fmt):
    chroma, _, sp, _ = FORMATS[fmt]
    return "444p" if chroma == 444 else ("420sp" if sp else "420p")


def sample_bytes(fmt):
    return 2 if FORMATS[fmt][1] > 8 else 1


def placements(fmt):
    return SEMI_PLACEMENTS if FORMATS[fmt][2] else PLANAR_PLACEMENTS


def plane_shapes(layout, h, w):
    """(rows, samples per row) of every plane of a picture"""
    return {"444p": [(h, w)] * 3, "420p": [(h, w), (h // 2, w // 2), (h // 2, w // 2)], "420sp": [(h, w), (h // 2, w)]}[layout]


def plane_geometry(layout, h, w, placement):
    """[(rows, samples per row, stride in samples, base offset in samples)] of every plane under a placement"""
    ey, ec, oy, ou, ov = placement
    shapes = plane_shapes(layout, h, w)
    extras, offsets = (ey, ec, ec), (oy, ou, ov)
    return [(r, n, n + extras[k], offsets[k]) for k, (r, n) in enumerate(shapes)]


# --------------------------------------------------------------------------------------------- the access-class rule
def expected_class(layout, es, pointers, ys, cs):
    """The rule of the header comment of dcvc_pixfmt.hip, restated: the widest class a of 8, 4, 2, 1 such that every plane's
    base and stride allow accesses of min(a, 16 / es) elements for the 8-element pieces of a row (luma, 4:4:4 chroma) and of
    min(max(a / 2, 1), 16 / es) for the 4-element pieces (planar 4:2:0 chroma); an interleaved row moves 4-element pieces of
    (U, V) pairs, an element of 2 es bytes, counted here as two samples.  es: bytes per sample; pointers: the planes' byte
    addresses (y, u[, v]); strides in samples.  It steers nothing: the case tables assert their own coverage with it."""
    def allows(samples, stride, ptrs):
        return stride % samples == 0 and all(p % (samples * es) == 0 for p in ptrs)

    for a in (8, 4, 2):
        w8, w4 = min(a, 16 // es), min(max(a // 2, 1), 16 // es)
        ok = allows(w8, ys, pointers[:1])
        if layout == "444p":
            ok = ok and allows(w8, cs, pointers[1:3])
        elif layout == "420p":
            ok = ok and allows(w4, cs, pointers[1:3])
        else:
            ok = ok and allows(2 * min(max(a // 2, 1), 16 // (2 * es)), cs, pointers[1:2])
        if ok:
            return a
    return 1


def case_class(layout, es, h, w, placement):
    """the class of a case whose regions start `offset` bytes past a 256-byte boundary (guarded / placed below)"""
    geo = plane_geometry(layout, h, w, placement)
    return expected_class(layout, es, [g[3] * es for g in geo], geo[0][2], geo[1][2])


def classes_reached(layout, es, cases):
    """the classes the cases (h, w, placement) with a picture wider than 8 reach: only there does a vector body sit next to
    a scalar tail or a second piece"""
    return {case_class(layout, es, h, w, pl) for h, w, pl in cases if w > 8}


# --------------------------------------------------------------------------------------------- device buffers
def plane_nbytes(rows, row_bytes, pitch_bytes):
    return (rows - 1) * pitch_bytes + row_bytes


def plane_mask(rows, row_bytes, pitch_bytes):
    """the bytes of a pitched plane that hold samples; the pitch gap of every row is not among them"""
    m = np.zeros(plane_nbytes(rows, row_bytes, pitch_bytes), bool)
    for r in range(rows):
        m[r * pitch_bytes:r * pitch_bytes + row_bytes] = True
    return m


def plane_rows(region, rows, row_bytes, pitch_bytes, dtype):
    """the samples [rows, row_bytes / itemsize] of a pitched plane held in the bytes `region`"""
    out = np.stack([region[r * pitch_bytes:r * pitch_bytes + row_bytes] for r in range(rows)])
    return np.ascontiguousarray(out).view(dtype)


class Guarded:
    """A uint8 device buffer filled with `fill`; the region of nbytes starts `offset` bytes past a 256-byte boundary and has
    at least GUARD canary bytes in front of and behind it.  ptr: the region's address; read(): the region's bytes on the
    host; check(written): every byte that is not a written sample still holds the fill - the pitch gaps, the bytes before
    the first sample and the bytes after the last one."""

    def __init__(self, nbytes, offset, fill):
        import torch
        self.nbytes, self.fill = nbytes, fill
        self.buf = torch.full((GUARD + 256 + offset + nbytes + GUARD,), fill, dtype=torch.uint8, device="cuda")
        base = self.buf.data_ptr()
        self.start = GUARD + (-(base + GUARD)) % 256 + offset
        self.ptr = base + self.start
        assert (self.ptr - offset) % 256 == 0 and self.start >= GUARD and self.buf.numel() - self.start - nbytes >= GUARD
        self._host = None

    def _all(self):
        if self._host is None:
            self._host = self.buf.cpu().numpy()
        return self._host

    def read(self):
        return self._all()[self.start:self.start + self.nbytes]

    def check(self, written=None):
        """written: a boolean mask over the region (True: a sample the launch may write); None: the whole region"""
        stray = self._all() != self.fill
        region = stray[self.start:self.start + self.nbytes]
        if written is not None:
            assert written.shape == region.shape
            where = np.flatnonzero(region & ~written)
            assert where.size == 0, f"{where.size} bytes between the samples were written, the first at region byte {where[0]}"
        front, back = np.flatnonzero(stray[:self.start]), np.flatnonzero(stray[self.start + self.nbytes:])
        assert front.size == 0, f"{front.size} bytes in front of the region were written, the nearest {self.start - front[-1]} before it"
        assert back.size == 0, f"{back.size} bytes behind the region were written, the first {back[0]} past its end"


def guarded(nbytes, offset, fill):
    return Guarded(nbytes, offset, fill)


class Placed:
    """A read-only source: `image` (bytes) `offset` bytes past a 256-byte boundary, random junk of `rng` around it"""

    def __init__(self, image, offset, rng):
        import torch
        n = image.size
        self.buf = torch.empty((GUARD + 256 + offset + n + GUARD,), dtype=torch.uint8, device="cuda")
        base = self.buf.data_ptr()
        start = GUARD + (-(base + GUARD)) % 256 + offset
        host = rng.integers(0, 256, self.buf.numel(), dtype=np.uint8)
        host[start:start + n] = image
        self.buf.copy_(torch.from_numpy(host))
        self.ptr = base + start
        assert (self.ptr - offset) % 256 == 0


def pitched_image(plane, stride, rng):
    """the bytes of `plane` [rows, n] laid out with `stride` samples per row, junk of `rng` in the pitch gaps"""
    rows, n = plane.shape
    es = plane.dtype.itemsize
    img = rng.integers(0, 256, plane_nbytes(rows, n * es, stride * es), dtype=np.uint8)
    for r in range(rows):
        img[r * stride * es:r * stride * es + n * es] = np.ascontiguousarray(plane[r]).view(np.uint8)
    return img


# --------------------------------------------------------------------------------------------- pictures and comparators
def tie_values(max_val, dtype):
    """values v of `dtype` whose fp32 product v * max_val is an exact .5 tie: [below an even integer, below an odd one]
    (None where the storage type has no such value: fp16 with max_val 255 has 127.5 = 0.5 * 255 only)"""
    k = np.arange(max_val, dtype=np.int64)
    v = ((k + 0.5) / max_val).astype(dtype)
    hit = v.astype(F) * F(max_val) == (k + 0.5).astype(F)
    out = []
    for parity in (1, 0):                                   # k odd: k + 1, the integer above the tie, is even
        ks = k[hit & (k % 2 == parity)]
        out.append(v[ks[ks.size // 2]] if ks.size else None)
    return out


def random_picture(rng, h, w, dtype, max_val):
    """[3, h, w] in [-0.05, 1.05] (both clamps act), the ties of tie_values in the first two 2x2 blocks of every plane (so
    that the 4:2:0 chroma mean of the block is the tie too)"""
    pic = rng.uniform(-0.05, 1.05, (3, h, w)).astype(F).astype(dtype)
    for j, v in enumerate(tie_values(max_val, dtype)):
        if v is not None and 2 * j < w:
            pic[:, :2, 2 * j:2 * j + 2] = v
    return pic


def poisoned_frame(pic, Hp, Wp):
    """the model frame [1, 3, Hp, Wp] with the picture at its top left and NaN everywhere else"""
    _, h, w = pic.shape
    x = np.full((1, 3, Hp, Wp), np.nan, pic.dtype)
    x[0, :, :h, :w] = pic
    return x


def file_planes(planes, fmt):
    """low-bit-aligned planar planes (y, u, v) -> the planes of the format: interleaved chroma, shifted up if msb-aligned"""
    _, bits, sp, msb = FORMATS[fmt]
    y, u, v = planes
    out = [y, R.interleave(u, v)] if sp else [y, u, v]
    return [p << (16 - bits) for p in out] if msb else out


def load_ref_pad(planes, chroma, bits, dtype, pad_b, pad_r):
    """pixfmt_ref.load_ref with an explicit pad: the last row and column replicated"""
    x = R.load_ref(planes, chroma, bits, dtype, pad_to=1)[0]
    return np.ascontiguousarray(np.pad(x, ((0, 0), (0, pad_b), (0, pad_r)), mode="edge")[None])
