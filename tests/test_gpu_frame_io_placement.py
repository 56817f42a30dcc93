"""The frame I/O kernels of csrc/dcvc_pixfmt.hip and the plane kernel of csrc/dcvc_metrics.hip on pitched, offset and
guarded planes, called through the C entries (the Python wrappers cannot express a pitch or an offset on the store side):
  A  dcvc_frame_to_planes / dcvc_frame_to_metric_planes write planes with a pitch and a base offset, each in a buffer of its
     own with canaries around it and in the pitch gaps, from frames whose every element outside the picture is NaN
  B  dcvc_planes_to_frame reads such planes, junk around them and in their gaps, into a guarded frame with explicit pads
  C  the 8-bit planar and RGB entries and dcvc_frame_to_yuv420_planes against the restatement tests/frame_io_ref.py (pinned
     to the reference's fixtures on the CPU by tests/test_frame_io_ref_host.py) at tiny and odd sizes, odd pads, byte offsets
Everything is compared bit for bit.  The comparators of A and B are tests/pixfmt_ref.py's (pinned by test_pixfmt_host.py).
The case tables of A and B assert, at import and on the CPU, that they reach every access class of the kernels."""
import numpy as np
import pytest
import torch

import frame_io_place as P
import frame_io_ref as C
import pixfmt_ref as R
from opendcvc_amd import _lib
from opendcvc_amd import nn as L

pytestmark = pytest.mark.gpu

DTYPES = [(torch.float32, np.float32, "f32"), (torch.float16, np.float16, "f16")]
LOAD_PAD_B = {420: (0, 2, 6), 444: (0, 1, 5)}


def _pad16(h, w):
    return (-h) % 16, (-w) % 16


def _load_pads(chroma, h, w):
    """pad to 16; WO the next multiple of 8 and the one after it (pad_r 0 .. 15, wider than a small picture), pad_b small"""
    pb, r8 = LOAD_PAD_B[chroma], (-w) % 8
    return [_pad16(h, w), (pb[0], r8), (pb[1], r8 + 8), (pb[2], r8)]


STORE_CASES = {fmt: [(h, w, pl) for h, w in P.PICTURES[P.FORMATS[fmt][0]] for pl in P.placements(fmt)] for fmt in P.FORMATS}
# a load case has a pad too; picture i under placement j takes pad (i + j) % 4, so every picture meets all four
LOAD_CASES = {fmt: [(h, w, pl, _load_pads(P.FORMATS[fmt][0], h, w)[(i + j) % 4])
                    for i, (h, w) in enumerate(P.PICTURES[P.FORMATS[fmt][0]]) for j, pl in enumerate(P.placements(fmt))]
              for fmt in P.FORMATS}
# the metric entry takes no strides: a class follows from W and the three base pointers (offsets in floats)
METRIC_WIDTHS = {420: (8, 12, 10), 444: (8, 12, 10, 9)}
METRIC_HEIGHT = {420: 4, 444: 3}
METRIC_OFFSETS = [(0, 0, 0), (1, 1, 1), (2, 2, 2), (3, 3, 3), (0, 2, 2), (2, 0, 0), (0, 0, 2), (0, 1, 0), (0, 0, 1), (1, 0, 0),
                  (0, 2, 0), (2, 2, 0)]


def _metric_class(chroma, w, offsets):
    return P.expected_class("444p" if chroma == 444 else "420p", 4, [4 * o for o in offsets], w, w if chroma == 444 else w // 2)


# ---- coverage, asserted on the CPU when the module is imported (pytest --collect-only shows a failure here)
for _fmt in P.FORMATS:
    for _cases in (STORE_CASES[_fmt], [c[:3] for c in LOAD_CASES[_fmt]]):
        _got = P.classes_reached(P.layout_of(_fmt), P.sample_bytes(_fmt), _cases)
        assert _got == {8, 4, 2, 1}, f"{_fmt}: the placement table reaches the classes {sorted(_got)} only"
# The metric planes are tight (stride = W), so a class's access width always divides the row: a vector body never has a
# partial tail there, whatever the width, and every width counts for the coverage.  With 4-byte elements a piece moves at
# most 16 / 4 = 4 elements: classes 8 and 4 both move 8-element pieces as min(8, 4) = min(4, 4) = 4 floats and differ in the
# 4-element pieces of 4:2:0 chroma only (min(4, 4) = 4 against min(2, 4) = 2).  4:4:4 has no such piece, so whatever
# allows class 4 there allows class 8, and class 4 cannot be reached.
assert {_metric_class(420, w, o) for w in METRIC_WIDTHS[420] for o in METRIC_OFFSETS} == {8, 4, 2, 1}
assert {_metric_class(444, w, o) for w in METRIC_WIDTHS[444] for o in METRIC_OFFSETS} == {8, 2, 1}
# fp32 frames have a tie below an even and below an odd integer at every bit depth; fp16 ones at least the one at 0.5
for _bits in (8, 10, 12, 16):
    assert all(v is not None for v in P.tie_values((1 << _bits) - 1, np.float32))
    assert any(v is not None for v in P.tie_values((1 << _bits) - 1, np.float16))


def _same(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want)


def _frames(pic, geometries):
    """the picture as poisoned model frames on the device: [(tensor, Hp, Wp)]"""
    out = []
    for hp, wp in geometries:
        x = torch.from_numpy(P.poisoned_frame(pic, hp, wp)).cuda()
        assert x.data_ptr() % 16 == 0
        out.append((x, hp, wp))
    return out


def _store_geometries(h, w):
    """pad to 16, and the least check_frame8 allows: H rounded up to even, W to a multiple of 8"""
    return [(h + (-h) % 16, w + (-w) % 16), (h + h % 2, w + (-w) % 8)]


# =============================================================================================== A. stores
@pytest.mark.parametrize("tdt,ndt,name", DTYPES)
@pytest.mark.parametrize("fmt", sorted(P.FORMATS))
def test_store_writes_the_samples_and_nothing_else(fmt, tdt, ndt, name):
    chroma, bits, sp, msb = P.FORMATS[fmt]
    layout, es = P.layout_of(fmt), P.sample_bytes(fmt)
    sdt = np.uint16 if es == 2 else np.uint8
    lib, code = _lib.lib(), L.dtype_code(tdt)
    rng = np.random.default_rng(bits * 1000 + chroma)
    for h, w in P.PICTURES[chroma]:
        pic = P.random_picture(rng, h, w, ndt, (1 << bits) - 1)
        frames = _frames(pic, _store_geometries(h, w))
        want = P.file_planes(R.store_ref(P.poisoned_frame(pic, h, w), h, w, chroma, bits), fmt)
        for pl in P.placements(fmt):
            geo = P.plane_geometry(layout, h, w, pl)
            for (x, hp, wp), fill in zip(frames, P.FILLS):                  # the same planes from both frame geometries
                bufs = [P.guarded(P.plane_nbytes(r, n * es, s * es), o * es, fill) for r, n, s, o in geo]
                ptrs = [b.ptr for b in bufs] + [None] * (3 - len(bufs))
                rc = lib.dcvc_frame_to_planes(code, chroma, bits, sp, msb, x.data_ptr(), hp, wp, h, w, *ptrs, geo[0][2], geo[1][2],
                                              L._stream())
                assert rc == 0, (h, w, pl, lib.dcvc_last_error())
                for b, t, (r, n, s, o) in zip(bufs, want, geo):
                    got = P.plane_rows(b.read(), r, n * es, s * es, sdt)
                    assert _same(got, t), (h, w, pl, hp, wp, int((got != t).sum()))
                    b.check(P.plane_mask(r, n * es, s * es))
                    if msb:
                        assert not (got & ((1 << (16 - bits)) - 1)).any()


@pytest.mark.parametrize("tdt,ndt,name", DTYPES)
@pytest.mark.parametrize("bits", [10, 16])
@pytest.mark.parametrize("chroma", [420, 444])
def test_metric_planes_at_float_offsets(chroma, bits, tdt, ndt, name):
    lib, code = _lib.lib(), L.dtype_code(tdt)
    h = METRIC_HEIGHT[chroma]
    rng = np.random.default_rng(bits + chroma)
    for w in METRIC_WIDTHS[chroma]:
        pic = P.random_picture(rng, h, w, ndt, (1 << bits) - 1)
        frames = _frames(pic, _store_geometries(h, w))
        want = R.metric_planes_ref(P.poisoned_frame(pic, h, w), h, w, chroma, bits)
        for offsets in METRIC_OFFSETS:
            for (x, hp, wp), fill in zip(frames, P.FILLS):
                bufs = [P.guarded(t.size * 4, 4 * o, fill) for t, o in zip(want, offsets)]
                rc = lib.dcvc_frame_to_metric_planes(code, chroma, (1 << bits) - 1, x.data_ptr(), hp, wp, h, w,
                                                     *[b.ptr for b in bufs], L._stream())
                assert rc == 0, (w, offsets, lib.dcvc_last_error())
                for b, t in zip(bufs, want):
                    assert _same(b.read().view(np.float32).reshape(t.shape), t), (w, offsets, hp, wp)
                    b.check()


def test_refused_placements_leave_the_planes_alone():
    """the three refusals that concern placement: a 16-bit plane at an odd address, an interleaved plane that is not aligned
    to a (U, V) pair, an odd interleaved stride; each returns negative, names the entry and writes nothing"""
    lib = _lib.lib()
    h, w = 4, 12
    x = torch.zeros((1, 3, 16, 16), dtype=torch.float16, device="cuda")
    #        format, byte offsets of (y, u / uv, v), c_stride
    cases = [("yuv420p10le", (1, 0, 0), w // 2), ("yuv420p10le", (0, 0, 1), w // 2), ("nv12", (0, 1, 0), w),
             ("p010le", (0, 2, 0), w), ("nv12", (0, 0, 0), w + 1), ("p010le", (0, 0, 0), w + 1)]
    for fmt, offs, cs in cases:
        chroma, bits, sp, msb = P.FORMATS[fmt]
        es = P.sample_bytes(fmt)
        shapes = P.plane_shapes(P.layout_of(fmt), h, w)
        strides = [w, cs, cs]
        bufs = [P.guarded(P.plane_nbytes(r, n * es, strides[k] * es), offs[k], P.FILLS[0]) for k, (r, n) in enumerate(shapes)]
        ptrs = [b.ptr for b in bufs] + [None] * (3 - len(bufs))
        rc = lib.dcvc_frame_to_planes(L.dtype_code(x.dtype), chroma, bits, sp, msb, x.data_ptr(), 16, 16, h, w, *ptrs, w, cs, L._stream())
        assert rc < 0 and b"dcvc_frame_to_planes" in lib.dcvc_last_error(), (fmt, offs, cs)
        out = P.guarded(3 * 16 * 16 * 2, 0, P.FILLS[1])
        rc = lib.dcvc_planes_to_frame(L.dtype_code(x.dtype), chroma, bits, sp, msb, *ptrs, w, cs, h, w, 12, 4, out.ptr, L._stream())
        assert rc < 0 and b"dcvc_planes_to_frame" in lib.dcvc_last_error(), (fmt, offs, cs)
        torch.cuda.synchronize()
        for b in bufs + [out]:
            b.check(np.zeros(b.nbytes, bool))


# =============================================================================================== B. loads
@pytest.mark.parametrize("tdt,ndt,name", DTYPES)
@pytest.mark.parametrize("fmt", sorted(P.FORMATS))
def test_load_reads_the_samples_and_nothing_else(fmt, tdt, ndt, name):
    chroma, bits, sp, msb = P.FORMATS[fmt]
    layout, es = P.layout_of(fmt), P.sample_bytes(fmt)
    lib, code = _lib.lib(), L.dtype_code(tdt)
    et = np.dtype(ndt).itemsize
    rng = np.random.default_rng(bits * 2000 + chroma)
    sources = {}
    for ci, (h, w, pl, (pad_b, pad_r)) in enumerate(LOAD_CASES[fmt]):
        if (h, w) not in sources:
            planes = [rng.integers(0, 1 << bits, s).astype(R.sample_dtype(bits)) for s in P.plane_shapes("444p" if chroma == 444 else "420p", h, w)]
            planes[0].flat[0], planes[0].flat[-1] = (1 << bits) - 1, 0
            sources[h, w] = planes
        planes = sources[h, w]
        want = P.load_ref_pad(planes, chroma, bits, ndt, pad_b, pad_r)
        ho, wo = h + pad_b, w + pad_r
        geo = P.plane_geometry(layout, h, w, pl)
        for run, fill in enumerate(P.FILLS):                                # two runs, different junk everywhere
            junk = np.random.default_rng(1000 * ci + run)
            fp = P.file_planes(planes, fmt)
            if msb:                                                         # (the bits below the sample are ignored)
                fp = [p | junk.integers(0, 1 << (16 - bits), p.shape).astype(p.dtype) for p in fp]
            srcs = [P.Placed(P.pitched_image(p, s, junk), o * es, junk) for p, (r, n, s, o) in zip(fp, geo)]
            out = P.guarded(3 * ho * wo * et, 16 * (ci % 2), fill)
            ptrs = [s.ptr for s in srcs] + [None] * (3 - len(srcs))
            rc = lib.dcvc_planes_to_frame(code, chroma, bits, sp, msb, *ptrs, geo[0][2], geo[1][2], h, w, pad_b, pad_r, out.ptr,
                                          L._stream())
            assert rc == 0, (h, w, pl, pad_b, pad_r, lib.dcvc_last_error())
            got = out.read().view(ndt).reshape(1, 3, ho, wo)
            assert _same(got, want), (h, w, pl, pad_b, pad_r, run, int((got != want).sum()))
            out.check()


# =============================================================================================== C. 8-bit planar and RGB
YUV_PICTURES = [(2, 2), (2, 6), (6, 2), (10, 22), (18, 34)]
RGB_PICTURES = [(1, 1), (3, 5), (7, 9), (16, 24)]
YUV_PADS = [(b, r) for b in (0, 2, 14) for r in (0, 2, 14)] + [(b, r) for b in (1, 3) for r in (1, 3)]     # (odd pads are legal)
RGB_PADS = [(b, r) for b in (0, 3, 14) for r in (0, 3, 14)]
BYTE_OFFSETS = [(0, 1, 3), (1, 3, 0), (3, 0, 1)]                   # uint8 planes sit anywhere


def _roomy(h, w):
    """frame geometries of the store entries, which ask only that the frame holds the picture: tight and roomy"""
    return [(h, w), (h + 3, w + 5)]


@pytest.mark.parametrize("tdt,ndt,name", DTYPES)
def test_yuv420_to_frame_at_tiny_sizes_and_any_pad(tdt, ndt, name):
    lib, code, et = _lib.lib(), L.dtype_code(tdt), np.dtype(ndt).itemsize
    rng = np.random.default_rng(420)
    for h, w in YUV_PICTURES:
        planes = [rng.integers(0, 256, s, dtype=np.uint8) for s in ((h, w), (h // 2, w // 2), (h // 2, w // 2))]
        planes[0].flat[0], planes[0].flat[-1] = 255, 0
        for ci, (pad_b, pad_r) in enumerate(YUV_PADS):
            srcs = [P.Placed(p.ravel(), o, rng) for p, o in zip(planes, BYTE_OFFSETS[ci % 3])]
            ho, wo = h + pad_b, w + pad_r
            out = P.guarded(3 * ho * wo * et, et, P.FILLS[ci % 2])
            rc = lib.dcvc_yuv420_to_frame(code, *[s.ptr for s in srcs], h, w, pad_b, pad_r, out.ptr, L._stream())
            assert rc == 0, lib.dcvc_last_error()
            got = out.read().view(ndt).reshape(1, 3, ho, wo)
            assert _same(got, C.yuv420_to_frame(*planes, ndt, pad_b, pad_r)), (h, w, pad_b, pad_r)
            out.check()


@pytest.mark.parametrize("tdt,ndt,name", DTYPES)
def test_rgb_to_frame_at_odd_sizes_and_any_pad(tdt, ndt, name):
    lib, code, et = _lib.lib(), L.dtype_code(tdt), np.dtype(ndt).itemsize
    rng = np.random.default_rng(709)
    for h, w in RGB_PICTURES:
        rgb = rng.integers(0, 256, (3, h, w), dtype=np.uint8)
        rgb[:, 0, 0], rgb[:, -1, -1] = (255, 0, 255), (0, 255, 1)
        for ci, (pad_b, pad_r) in enumerate(RGB_PADS):
            src = P.Placed(rgb.ravel(), (0, 1, 3)[ci % 3], rng)
            ho, wo = h + pad_b, w + pad_r
            out = P.guarded(3 * ho * wo * et, et, P.FILLS[ci % 2])
            rc = lib.dcvc_rgb_to_frame(code, src.ptr, h, w, pad_b, pad_r, out.ptr, L._stream())
            assert rc == 0, lib.dcvc_last_error()
            got = out.read().view(ndt).reshape(1, 3, ho, wo)
            assert _same(got, C.rgb_to_frame(rgb, ndt, pad_b, pad_r)), (h, w, pad_b, pad_r)
            out.check()


@pytest.mark.parametrize("tdt,ndt,name", DTYPES)
def test_frame_to_yuv420_and_its_planes_from_poisoned_frames(tdt, ndt, name):
    lib, code, et = _lib.lib(), L.dtype_code(tdt), np.dtype(ndt).itemsize
    rng = np.random.default_rng(8)
    for pi, (h, w) in enumerate(YUV_PICTURES):
        pic = P.random_picture(rng, h, w, ndt, 255)
        tight = P.poisoned_frame(pic, h, w)
        want_planes = C.yuv420_planes(tight, h, w)
        for (x, hp, wp), fill in zip(_frames(pic, _roomy(h, w)), P.FILLS):
            for round_uv in (0, 1):
                want = C.frame_to_yuv420(tight, h, w, round_uv)
                for offs in BYTE_OFFSETS:
                    bufs = [P.guarded(t.size, o, fill) for t, o in zip(want, offs)]
                    rc = lib.dcvc_frame_to_yuv420(code, x.data_ptr(), hp, wp, h, w, round_uv, *[b.ptr for b in bufs], L._stream())
                    assert rc == 0, lib.dcvc_last_error()
                    for b, t, k in zip(bufs, want, "yuv"):
                        assert _same(b.read().reshape(t.shape), t), (h, w, hp, wp, round_uv, offs, k)
                        b.check()
            bufs = [P.guarded(t.size * et, et, fill) for t in want_planes]         # one element past a 16-byte boundary
            rc = lib.dcvc_frame_to_yuv420_planes(code, x.data_ptr(), hp, wp, h, w, *[b.ptr for b in bufs], L._stream())
            assert rc == 0, lib.dcvc_last_error()
            for b, t, k in zip(bufs, want_planes, "yuv"):
                assert _same(b.read().view(ndt).reshape(t.shape), t), (h, w, hp, wp, k)
                b.check()


@pytest.mark.parametrize("tdt,ndt,name", DTYPES)
def test_frame_to_rgb_from_poisoned_frames(tdt, ndt, name):
    lib, code, et = _lib.lib(), L.dtype_code(tdt), np.dtype(ndt).itemsize
    rng = np.random.default_rng(9)
    for h, w in RGB_PICTURES:
        pic = P.random_picture(rng, h, w, ndt, 255)
        want = C.frame_to_rgb(P.poisoned_frame(pic, h, w), h, w)
        for (x, hp, wp), fill in zip(_frames(pic, _roomy(h, w)), P.FILLS):
            out = P.guarded(want.size * et, et, fill)
            rc = lib.dcvc_frame_to_rgb(code, x.data_ptr(), hp, wp, h, w, out.ptr, L._stream())
            assert rc == 0, lib.dcvc_last_error()
            assert _same(out.read().view(ndt).reshape(want.shape), want), (h, w, hp, wp)
            out.check()
