"""4:2:2 frame I/O (csrc/dcvc_pix422.hip, opendcvc_amd/pix422.py, docs/pixel_formats_422.md) as far as a GPU-less host can
check it: the entries are declared, bound and exported, argument errors come back without a device, the layouts of the numpy
restatement are pinned against literal bytes, the formats parse, the reader delivers each format's frames, the source types
reach run_one_point, and the restatement agrees with the 4:4:4 one it continues."""
import ctypes
import os
import re

import numpy as np
import pytest

import pix422_ref as R2
import pixfmt_ref as R
from opendcvc_amd import _lib, harness, pix422
from opendcvc_amd.pipeline import PixelFormat
from opendcvc_amd.pix422 import FORMATS_422, Format422, Raw422Reader

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dcvc_v210_row_bytes", "dcvc_yuv422_to_frame", "dcvc_frame_to_yuv422")
PLANAR, UYVY, YUYV, V210 = 0, 1, 2, 3


def test_entries_are_declared_bound_and_exported():
    header = open(os.path.join(REPO, "include", "dcvc_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert os.path.exists(_lib.LIB_PATH), "libdcvc_amd.so not built (run __graft_entry__.build())"
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, code), f"{name} not declared in dcvc_amd.h"
        assert name in _lib.EXPORTS and hasattr(L, name), name
    for k, name in enumerate(("PLANAR", "UYVY", "YUYV", "V210")):
        assert re.search(r"\bDCVC_422_%s\s*=\s*%d\b" % (name, k), code), name
    assert (pix422.PLANAR, pix422.UYVY, pix422.YUYV, pix422.V210) == (0, 1, 2, 3)
    assert re.search(r"#define\s+DCVC_ABI_VERSION\s+1\b", header) and _lib.lib().dcvc_abi_version() == 1


def test_v210_row_bytes():
    lib = _lib.lib()
    for w, want in ((2, 128), (6, 128), (46, 128), (48, 128), (50, 256), (1920, 5120), (3840, 10240)):
        assert lib.dcvc_v210_row_bytes(w) == want == R2.row_bytes("v210", w) == Format422.parse("v210").row_bytes(w)
    assert lib.dcvc_v210_row_bytes(0) <= 0 and lib.dcvc_v210_row_bytes(-6) <= 0


# a 64-byte-aligned host buffer stands in for every pointer: each call below must be refused before anything is launched
_BUF = ctypes.create_string_buffer(8192 + 64)
_PTR = (ctypes.addressof(_BUF) + 63) & ~63


def _strides(layout, W, ys, cs):
    if ys is None:
        ys = W if layout == PLANAR else (R2.row_bytes("v210", W) if layout == V210 and W > 0 and W % 2 == 0 else 2 * max(W, 64))
    return ys, (W // 2 if cs is None else cs)


def _load(layout=PLANAR, bits=None, y=_PTR, u=_PTR, v=_PTR, ys=None, cs=None, H=4, W=16, pb=0, pr=0, out=_PTR, dtype=_lib.F16):
    bits = {PLANAR: 10, UYVY: 8, YUYV: 8, V210: 10}.get(layout, 8) if bits is None else bits
    ys, cs = _strides(layout, W, ys, cs)
    return _lib.lib().dcvc_yuv422_to_frame(dtype, layout, bits, y, u, v, ys, cs, H, W, pb, pr, out, None)


def _store(layout=PLANAR, bits=None, y=_PTR, u=_PTR, v=_PTR, ys=None, cs=None, H=4, W=16, Hp=4, Wp=16, x=_PTR, dtype=_lib.F16):
    bits = {PLANAR: 10, UYVY: 8, YUYV: 8, V210: 10}.get(layout, 8) if bits is None else bits
    ys, cs = _strides(layout, W, ys, cs)
    return _lib.lib().dcvc_frame_to_yuv422(dtype, layout, bits, x, Hp, Wp, H, W, y, u, v, ys, cs, None)


@pytest.mark.parametrize("call", [_load, _store])
def test_argument_errors_need_no_device(call):
    bad = [dict(W=15), dict(layout=UYVY, W=15), dict(layout=V210, W=15),            # an odd width
           dict(H=0), dict(W=0), dict(H=-1), dict(W=-2),
           dict(layout=UYVY, bits=9), dict(layout=YUYV, bits=10), dict(layout=V210, bits=8),
           dict(layout=V210, bits=12), dict(bits=7), dict(bits=17),                 # bit depths
           dict(layout=4), dict(layout=-1),                                         # an unknown layout
           dict(y=None), dict(u=None), dict(v=None), dict(layout=UYVY, y=None), dict(layout=V210, y=None),
           dict(ys=15), dict(cs=7), dict(layout=UYVY, ys=28), dict(layout=YUYV, ys=31), dict(layout=V210, ys=112),
           dict(layout=UYVY, y=_PTR + 2), dict(layout=YUYV, y=_PTR + 1), dict(layout=UYVY, ys=34),
           dict(layout=V210, y=_PTR + 8), dict(layout=V210, y=_PTR + 4), dict(layout=V210, ys=136),
           dict(bits=10, y=_PTR + 1), dict(dtype=_lib.U8)]
    bad += ([dict(out=None), dict(pr=4), dict(pb=-1), dict(pr=-8), dict(out=_PTR + 8)] if call is _load else
            [dict(x=None), dict(Wp=20), dict(Wp=8), dict(Hp=3), dict(x=_PTR + 8)])
    for kw in bad:
        assert call(**kw) == -1, kw
        assert _lib.lib().dcvc_last_error(), kw


def test_packed_layouts_take_null_chroma_pointers_and_planar_does_not():
    """u / v NULL is an error for the planar layout only: with a packed layout the same call fails on a LATER check (the NULL
    frame), whose message it then carries"""
    lib = _lib.lib()
    for layout in (UYVY, YUYV, V210):
        assert _load(layout=layout, u=None, v=None, out=None) == -1 and b"output" in lib.dcvc_last_error()
        assert _store(layout=layout, u=None, v=None, x=None) == -1 and b"null pointer" in lib.dcvc_last_error()
    assert _load(u=None, out=None) == -1 and b"null plane" in lib.dcvc_last_error()
    assert _store(v=None, x=None) == -1 and b"null plane" in lib.dcvc_last_error()


def test_metric_planes_take_422_and_keep_their_refusals():
    lib = _lib.lib()
    metric = lambda chroma=422, max_val=1023, H=5, W=16, y=_PTR, x=_PTR, Wp=16: lib.dcvc_frame_to_metric_planes(
        _lib.F16, chroma, max_val, x, 8, Wp, H, W, y, _PTR, _PTR, None)
    for kw in (dict(W=15), dict(chroma=400), dict(chroma=421), dict(max_val=0), dict(max_val=65536), dict(y=None), dict(x=None),
               dict(Wp=20), dict(H=9), dict(chroma=420, H=5)):
        assert metric(**kw) == -1, kw
    # the 4:2:0 / 4:4:4 entries still refuse 4:2:2
    assert lib.dcvc_planes_to_frame(_lib.F16, 422, 10, 0, 0, _PTR, _PTR, _PTR, 32, 16, 16, 32, 0, 0, _PTR, None) == -1
    assert lib.dcvc_frame_to_planes(_lib.F16, 422, 10, 0, 0, _PTR, 16, 32, 16, 32, _PTR, _PTR, _PTR, 32, 16, None) == -1


# ------------------------------------------------------------------------------------------- the layouts, in literal bytes
V210_WORDS = (0x20000500, 0x00340402, 0x10201201, 0x00680805)
V210_BYTES = bytes.fromhex("00050020 02043400 01122010 05086800".replace(" ", ""))
V210_Y = np.array([[1, 2, 3, 4, 5, 6]], np.uint16)
V210_CB = np.array([[0x100, 0x101, 0x102]], np.uint16)
V210_CR = np.array([[0x200, 0x201, 0x202]], np.uint16)


def test_known_answers_of_the_layouts():
    assert np.array(V210_WORDS, "<u4").tobytes() == V210_BYTES
    (s,) = R2.pack([V210_Y, V210_CB, V210_CR], "v210")
    assert s.dtype == np.uint8 and s.shape == (1, 128)
    assert s[0, :16].tobytes() == V210_BYTES and not s[0, 16:].any()
    for got, want in zip(R2.unpack([s], "v210", 6), (V210_Y, V210_CB, V210_CR)):
        assert np.array_equal(got, want)
    # a row narrower than its last group: the samples past the picture are zero, and unpack does not hand them on
    (s4,) = R2.pack([V210_Y[:, :4], V210_CB[:, :2], V210_CR[:, :2]], "v210")
    assert s4[0, :16].view("<u4").tolist() == [0x20000500, 0x00340402, 0x00001201, 0] and not s4[0, 16:].any()
    assert [p.shape for p in R2.unpack([s], "v210", 4)] == [(1, 4), (1, 2), (1, 2)]
    # 8 pixels: the second group starts at byte 16
    y8 = np.arange(1, 9, dtype=np.uint16)[None]
    (s8,) = R2.pack([y8, V210_CB[:, [0, 1, 2, 0]], V210_CR[:, [0, 1, 2, 0]]], "v210")
    assert s8[0, :16].tobytes() == V210_BYTES and s8[0, 16:24].view("<u4").tolist() == [0x100 | 7 << 10 | 0x200 << 20, 8]
    pair = [np.array([[1, 2]], np.uint8), np.array([[3]], np.uint8), np.array([[4]], np.uint8)]
    assert R2.pack(pair, "uyvy422")[0].tobytes() == bytes([3, 1, 4, 2])
    assert R2.pack(pair, "yuyv422")[0].tobytes() == bytes([1, 3, 2, 4])
    for name in ("uyvy422", "yuyv422"):
        for got, want in zip(R2.unpack(R2.pack(pair, name), name, 2), pair):
            assert np.array_equal(got, want)
    for w, want in ((2, 128), (6, 128), (46, 128), (48, 128), (50, 256)):
        assert R2.row_bytes("v210", w) == want
    assert R2.row_bytes("uyvy422", 6) == 12 and R2.row_bytes("yuv422p10le", 6) == 12 and R2.row_bytes("yuv422p", 6) == 6


def test_unpack_422_agrees_with_the_literal_bytes():
    """the torch glue of the measuring side (CPU tensors here) reads the same layouts"""
    import torch
    s = np.zeros((1, 128), np.uint8)
    s[0, :16] = np.frombuffer(V210_BYTES, np.uint8)
    got = pix422.unpack_422([torch.from_numpy(s)], "v210", 6)
    for g, want in zip(got, (V210_Y, V210_CB, V210_CR)):
        assert g.dtype == torch.uint16 and np.array_equal(g.view(torch.int16).numpy().astype(np.uint16), want)
    for name, raw in (("uyvy422", [3, 1, 4, 2]), ("yuyv422", [1, 3, 2, 4])):
        y, u, v = pix422.unpack_422(torch.tensor([raw + [0, 0]], dtype=torch.uint8), name, 2)       # (a pitch of 6)
        assert (y.tolist(), u.tolist(), v.tolist()) == ([[1, 2]], [[3]], [[4]])
    rng = np.random.default_rng(5)
    for name in R2.FORMATS:
        planes = R2.random_planes(rng, 3, 26, R2.bits_of(name))
        frame = R2.pack(planes, name)
        as_torch = [torch.from_numpy(p.view(np.int16) if p.dtype.itemsize == 2 else p) for p in frame]
        for g, want in zip(harness.source_planes(as_torch, Format422.parse(name), 26), planes):
            g = g.view(torch.int16).numpy().view(np.uint16) if g.element_size() == 2 else g.numpy()
            assert np.array_equal(g, want), name


# ------------------------------------------------------------------------------------------- the Python table and reader
def test_format_422_parses_its_table_and_nothing_else():
    assert list(FORMATS_422) == ["yuv422p", "yuv422p10le", "yuv422p12le", "yuv422p16le", "uyvy422", "yuyv422", "v210"]
    assert set(FORMATS_422) == set(R2.FORMATS) and harness.SRC_TYPES_422 == tuple(FORMATS_422)
    for name, (packing, bits) in R2.FORMATS.items():
        f = Format422.parse(name)
        assert (f.name, f.packing, f.bit_depth, f.chroma, f.layout) == (name, packing, bits, 422, R2.LAYOUT[packing])
        assert f.max_val == (1 << bits) - 1 and f.sample_bytes == (2 if bits > 8 else 1) and Format422.parse(f) is f
        assert f.row_bytes(50) == R2.row_bytes(name, 50)
        assert f.frame_bytes(7, 50) == sum(p.nbytes for p in R2.pack(R2.random_planes(np.random.default_rng(0), 7, 50, bits), name))
        with pytest.raises(ValueError):
            f.frame_bytes(7, 49)
    for name in ("yuv420", "png", "rgb24", "yuv444p", "yuv420p10le", "nv16", "p210le", "y210le", "yuv422p10be", "", None, "V210"):
        with pytest.raises(ValueError):
            Format422.parse(name)
    for args in (("x", "uyvy", 10), ("x", "v210", 8), ("x", "planar", 7), ("x", "planar", 17), ("x", "nv16", 8)):
        with pytest.raises(ValueError):
            Format422(*args)
    with pytest.raises(ValueError):
        PixelFormat.parse("yuv422p")                                     # 4:2:2 has its own table
    assert len(harness.SRC_TYPES) == 11 and not set(harness.SRC_TYPES) & set(FORMATS_422)


@pytest.mark.parametrize("name", sorted(R2.FORMATS))
def test_raw_422_reader_delivers_the_files_frames(tmp_path, name):
    f = Format422.parse(name)
    h, w, n = 5, 50, 3
    rng = np.random.default_rng(len(name))
    frames = [R2.pack(R2.random_planes(rng, h, w, f.bit_depth), name) for _ in range(n)]
    path = str(tmp_path / "clip.raw")
    with open(path, "wb") as fp:
        for frame in frames:
            for p in frame:
                fp.write(p.tobytes())
        fp.write(b"\0" * (f.frame_bytes(h, w) - 1))                     # a truncated last frame
    assert os.path.getsize(path) == (n + 1) * f.frame_bytes(h, w) - 1
    reader = Raw422Reader(path, w, h, name)
    for frame in frames:
        got = reader.read()
        assert len(got) == (1 if f.packed else 3)
        for g, p in zip(got, frame):
            assert g.dtype == p.dtype and g.shape == p.shape and np.array_equal(g, p)
        if f.packed:
            assert got[0].shape == (h, f.row_bytes(w))
    with pytest.raises(EOFError):
        reader.read()
    reader.close()
    with pytest.raises(ValueError):
        Raw422Reader(path, w + 1, h, name)


def test_src_type_parses_and_reaches_the_jobs_and_run_one_point(monkeypatch):
    ap = harness.build_parser()
    for name in FORMATS_422:
        for opt in ("--src-type", "--src_type"):
            assert ap.parse_args(f"--src a.yuv --width 64 --height 64 --frames 1 {opt} {name}".split()).src_type == name
    assert ap.parse_args("--src a.yuv --width 64 --height 64 --frames 1".split()).src_type == "yuv420"
    for name in ("rgb24", "nv16", "y210le"):
        with pytest.raises(SystemExit):
            ap.parse_args(f"--src a.yuv --width 64 --height 64 --frames 1 --src-type {name}".split())
    config = {"root_path": "/data", "test_classes": {
        "SDI": {"test": 1, "base_path": "sdi", "src_type": "v210", "sequences": {
            "a.v210": {"width": 64, "height": 62, "frames": 2, "intra_period": -1}}},
        "MEZZ": {"test": 1, "base_path": "mezz", "src_type": "yuv422p10le", "sequences": {
            "b.yuv": {"width": 64, "height": 64, "frames": 2, "intra_period": -1}}}}}
    jobs = harness.jobs_from_config(config, dict(qp_i=[10, 20]))
    assert [j["src_type"] for j in jobs] == ["v210"] * 2 + ["yuv422p10le"] * 2
    bad = {"root_path": "/data", "test_classes": {"X": dict(config["test_classes"]["SDI"], src_type="rgb24")}}
    with pytest.raises(ValueError, match="rgb24"):
        harness.jobs_from_config(bad, {})
    seen = []
    monkeypatch.setattr(harness, "run_one_point", lambda *a, **kw: seen.append((kw["src_type"], kw["rec_path"])) or {})
    harness.run_job(("i", "p"), jobs[0], {})
    harness.run_job(("i", "p"), jobs[2], {})
    assert seen == [("v210", None), ("yuv422p10le", None)]
    args = ap.parse_args("--src a.v210 --width 64 --height 62 --frames 1 --src-type v210".split())
    assert args.src_type == "v210"


def test_sources_have_one_row_chroma_lines_and_refuse_an_odd_width():
    for name in FORMATS_422:
        src = harness.make_source(name, "/nonexistent.raw", 64, 38)
        assert src.chroma_lines == 1 and (src.w, src.h) == (64, 38)
        with pytest.raises(ValueError, match=name):
            harness.make_source(name, "/nonexistent.raw", 63, 38)
        with pytest.raises(ValueError, match=name):
            harness.run_one_point(None, None, "/nonexistent.raw", 63, 64, 1, 0, src_type=name)
    with pytest.raises(ValueError, match="rgb24"):
        harness.run_one_point(None, None, "/nonexistent.yuv", 64, 64, 1, 0, src_type="rgb24")
    assert harness.make_source("yuv420p10le", "/nonexistent.raw", 64, 40).chroma_lines == 2


# ------------------------------------------------------------------------------------------- the restatement's identities
@pytest.mark.parametrize("name", sorted(R2.FORMATS))
def test_load_equals_the_444_load_of_doubled_chroma_and_store_inverts_it(name):
    bits = R2.bits_of(name)
    rng = np.random.default_rng(bits + len(name))
    for h, w in ((3, 22), (1, 2), (5, 50)):
        planes = R2.random_planes(rng, h, w, bits)
        frame = R2.pack(planes, name)
        doubled = [planes[0], np.repeat(planes[1], 2, axis=1), np.repeat(planes[2], 2, axis=1)]
        for dt in (np.float32, np.float16):
            x = R2.load_ref(frame, name, dt, w)
            assert x.dtype == dt and x.shape == (1, 3, h + (-h) % 16, w + (-w) % 16)
            assert np.array_equal(x, R.load_ref(doubled, 444, bits, dt))
            if dt == np.float16 and bits > 8:
                continue
            # fp16, 8 bits: s / 255 rounded to fp16 is off by at most 2^-11 relative, 255 * 2^-11 < 1/2 codes: rint finds s
            back = R2.store_ref(x, h, w, name)
            assert len(back) == len(frame)
            for b, f in zip(back, frame):
                assert b.dtype == f.dtype and np.array_equal(b, f)
        x = R2.load_ref(frame, name, np.float32, w, pad=(0, 8 - w % 8))
        assert x.shape == (1, 3, h, w + 8 - w % 8) and np.array_equal(x[0, :, :, w:], np.repeat(x[0, :, :, w - 1:w], 8 - w % 8, axis=2))


def test_the_host_path_metric_planes_are_the_restatements():
    import torch
    rng = np.random.default_rng(4)
    for dt in (np.float32, np.float16):
        x = rng.uniform(-0.05, 1.05, (1, 3, 48, 64)).astype(np.float32).astype(dt)
        for name in ("yuv422p", "uyvy422", "v210", "yuv422p16le"):
            f = Format422.parse(name)
            got = harness.pixfmt_metric_planes(torch.from_numpy(x), 37, 50, f)
            want = R2.metric_planes_ref(x, 37, 50, f.bit_depth)
            assert [tuple(g.shape) for g in got] == [(37, 50), (37, 25), (37, 25)]
            for g, wnt in zip(got, want):
                assert g.dtype == torch.float32 and np.array_equal(g.numpy(), wnt)


def test_host_metrics_of_a_packed_source_equal_the_planar_ones():
    """pixfmt_distortion on CPU tensors: a v210 surface against the same samples as yuv422p10le; a perfect reconstruction gives
    the cap; data_range is max_val and the combination (6 Y + U + V) / 8"""
    import torch
    rng = np.random.default_rng(9)
    h, w = 90, 182
    planes = R2.random_planes(rng, h, w, 10)
    x = torch.from_numpy(R2.load_ref(planes, "yuv422p10le", np.float32))
    planar = [torch.from_numpy(p.view(np.int16)).view(torch.uint16) for p in planes]
    surface = [torch.from_numpy(R2.pack(planes, "v210")[0])]
    a = harness.pixfmt_distortion(x, planar, Format422.parse("yuv422p10le"))
    assert a[0] == [99.9] * 4
    noisy = (x + torch.from_numpy(rng.normal(0, 0.01, tuple(x.shape)).astype(np.float32))).half()
    a = harness.pixfmt_distortion(noisy, planar, Format422.parse("yuv422p10le"), width=w)
    b = harness.pixfmt_distortion(noisy, surface, Format422.parse("v210"), width=w)
    assert a == b and 30 < a[0][1] < 50 and a[0][0] == (6 * a[0][1] + a[0][2] + a[0][3]) / 8
