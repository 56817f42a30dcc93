"""High-bit-depth / 4:4:4 / NV12 / P010 frame I/O (csrc/dcvc_pixfmt.hip, pipeline.PixelFormat, harness.RawVideoReader) as
far as a GPU-less host can check it: the entries are declared, bound and exported, argument errors come back without a
device, the formats parse, the reader delivers each format's planes, the source type reaches run_one_point, and the numpy
restatement the GPU tests compare with equals the reference family's reader / writer output sample for sample."""
import ctypes
import os
import re

import numpy as np
import pytest

import pixfmt_ref as R
from opendcvc_amd import _lib, harness
from opendcvc_amd.pipeline import PIXEL_FORMATS, PixelFormat

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dcvc_planes_to_frame", "dcvc_frame_to_planes", "dcvc_frame_to_metric_planes")
TABLE = {  # name: (chroma, bits, semi_planar, msb_aligned)
    "yuv420p10le": (420, 10, False, False), "yuv420p12le": (420, 12, False, False), "yuv420p16le": (420, 16, False, False),
    "yuv444p": (444, 8, False, False), "yuv444p10le": (444, 10, False, False), "yuv444p12le": (444, 12, False, False),
    "yuv444p16le": (444, 16, False, False), "nv12": (420, 8, True, False), "p010le": (420, 10, True, True)}


def test_entries_are_declared_bound_and_exported():
    header = open(os.path.join(REPO, "include", "dcvc_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert os.path.exists(_lib.LIB_PATH), "libdcvc_amd.so not built (run __graft_entry__.build())"
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, code), f"{name} not declared in dcvc_amd.h"
        assert name in _lib.EXPORTS and hasattr(L, name), name
    assert re.search(r"\bDCVC_U16\s*=\s*3\b", code) and _lib.U16 == 3
    assert re.search(r"\bDCVC_U8\s*=\s*2\b", code) and _lib.U8 == 2
    assert re.search(r"#define\s+DCVC_ABI_VERSION\s+1\b", header) and _lib.lib().dcvc_abi_version() == 1


# a 64-byte-aligned host buffer stands in for every pointer: each call below must be refused before anything is launched
_BUF = ctypes.create_string_buffer(4096 + 64)
_PTR = (ctypes.addressof(_BUF) + 63) & ~63


def _load(chroma=420, bits=10, sp=0, msb=0, y=_PTR, u=_PTR, v=_PTR, ys=None, cs=None, H=16, W=32, pb=0, pr=0, out=_PTR, dtype=_lib.F16):
    ys = W if ys is None else ys
    cs = (W if (chroma == 444 or sp) else W // 2) if cs is None else cs
    return _lib.lib().dcvc_planes_to_frame(dtype, chroma, bits, sp, msb, y, u, v, ys, cs, H, W, pb, pr, out, None)


def _store(chroma=420, bits=10, sp=0, msb=0, y=_PTR, u=_PTR, v=_PTR, ys=None, cs=None, H=16, W=32, Hp=16, Wp=32, x=_PTR, dtype=_lib.F16):
    ys = W if ys is None else ys
    cs = (W if (chroma == 444 or sp) else W // 2) if cs is None else cs
    return _lib.lib().dcvc_frame_to_planes(dtype, chroma, bits, sp, msb, x, Hp, Wp, H, W, y, u, v, ys, cs, None)


@pytest.mark.parametrize("call", [_load, _store])
def test_argument_errors_need_no_device(call):
    bad = [dict(H=15), dict(W=31), dict(H=15, W=31),                       # odd sizes with 4:2:0
           dict(bits=7), dict(bits=17), dict(bits=0),                      # bit depth outside 8 .. 16
           dict(bits=8, msb=1),                                            # msb_aligned with 8 bits
           dict(y=None), dict(u=None), dict(v=None), dict(sp=1, u=None),   # a NULL plane
           dict(ys=31), dict(cs=15), dict(chroma=444, cs=31), dict(sp=1, cs=30),   # a stride below the row length
           dict(chroma=422), dict(chroma=444, sp=1), dict(dtype=_lib.U8), dict(H=0), dict(W=0)]
    bad += [dict(out=None), dict(pr=4), dict(pb=-1)] if call is _load else [dict(x=None), dict(Wp=24), dict(Hp=8), dict(Wp=36)]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert _lib.lib().dcvc_last_error(), kw
    lib = _lib.lib()
    metric = lambda chroma=420, max_val=1023, H=16, W=32, y=_PTR, x=_PTR, Wp=32: lib.dcvc_frame_to_metric_planes(
        _lib.F16, chroma, max_val, x, 16, Wp, H, W, y, _PTR, _PTR, None)
    for kw in (dict(H=15), dict(W=31), dict(chroma=400), dict(max_val=0), dict(max_val=65536), dict(y=None), dict(x=None), dict(Wp=28)):
        assert metric(**kw) == -1, kw
    # the metric entries know the new element type and still refuse an unknown one (checked before the device is touched)
    for t in (4, -1):
        assert lib.dcvc_sse(t, _PTR, _lib.U16, _PTR, 16, _PTR, ctypes.cast(_PTR, ctypes.POINTER(ctypes.c_double)), None) == -1
    assert b"bad element types" in lib.dcvc_last_error()


def test_pixel_format_parses_the_table_and_nothing_else():
    assert set(PIXEL_FORMATS) == set(TABLE)
    for name, (chroma, bits, sp, msb) in TABLE.items():
        f = PixelFormat.parse(name)
        assert (f.name, f.chroma, f.bit_depth, f.semi_planar, f.msb_aligned) == (name, chroma, bits, sp, msb)
        assert f.max_val == (1 << bits) - 1 and f.sample_bytes == (2 if bits > 8 else 1)
        assert PixelFormat.parse(f) is f
        shapes = f.plane_shapes(70, 98)
        want = [(70, 98)] * 3 if chroma == 444 else ([(70, 98), (35, 98)] if sp else [(70, 98), (35, 49), (35, 49)])
        assert list(shapes) == want
        assert f.frame_bytes(70, 98) == 70 * 98 * (3 if chroma == 444 else 1.5) * f.sample_bytes
        if chroma == 420:
            for h, w in ((71, 98), (70, 97)):
                with pytest.raises(ValueError):
                    f.plane_shapes(h, w)
    for name in ("yuv420", "png", "rgb24", "yuv422p", "yuv420p10be", "p016le", "", None, "YUV444P"):
        with pytest.raises(ValueError):
            PixelFormat.parse(name)
    with pytest.raises(ValueError):
        PixelFormat("x", 420, 8, msb_aligned=True)
    with pytest.raises(ValueError):
        PixelFormat("x", 444, 10, semi_planar=True)


@pytest.mark.parametrize("name", sorted(TABLE))
def test_raw_video_reader_delivers_the_files_planes(tmp_path, name):
    f = PixelFormat.parse(name)
    h, w, n = 6, 10, 3
    rng = np.random.default_rng(len(name))
    dt = "<u2" if f.bit_depth > 8 else "u1"
    frames = [[rng.integers(0, f.max_val + 1, s).astype(dt) << (16 - f.bit_depth if f.msb_aligned else 0) for s in f.plane_shapes(h, w)]
              for _ in range(n)]
    path = str(tmp_path / "clip.raw")
    with open(path, "wb") as fp:
        for planes in frames:
            for p in planes:
                fp.write(p.astype(dt).tobytes())
        fp.write(b"\0" * (f.frame_bytes(h, w) - 1))                     # a truncated last frame
    assert os.path.getsize(path) == (n + 1) * f.frame_bytes(h, w) - 1
    reader = harness.RawVideoReader(path, w, h, name)
    for planes in frames:
        got = reader.read()
        assert len(got) == (2 if f.semi_planar else 3)                  # (semi-planar stays semi-planar)
        for g, p in zip(got, planes):
            assert g.dtype == np.dtype(dt) and g.shape == p.shape and np.array_equal(g, p)
    with pytest.raises(EOFError):
        reader.read()
    reader.close()
    if f.chroma == 420:
        with pytest.raises(ValueError):
            harness.RawVideoReader(path, w + 1, h, name)


def test_src_type_parses_and_reaches_the_jobs_and_run_one_point(monkeypatch):
    ap = harness.build_parser()
    for name in TABLE:
        for opt in ("--src-type", "--src_type"):
            assert ap.parse_args(f"--src a.yuv --width 64 --height 64 --frames 1 {opt} {name}".split()).src_type == name
    assert ap.parse_args("--src a.yuv --width 64 --height 64 --frames 1".split()).src_type == "yuv420"
    with pytest.raises(SystemExit):
        ap.parse_args("--src a.yuv --width 64 --height 64 --frames 1 --src-type rgb24".split())
    config = {"root_path": "/data", "test_classes": {
        "HW": {"test": 1, "base_path": "hw", "src_type": "p010le", "sequences": {
            "a.yuv": {"width": 64, "height": 64, "frames": 2, "intra_period": -1}}},
        "UVG": {"test": 1, "base_path": "uvg", "src_type": "yuv420p10le", "sequences": {
            "b.yuv": {"width": 64, "height": 64, "frames": 2, "intra_period": -1}}}}}
    jobs = harness.jobs_from_config(config, dict(qp_i=[10, 20]))
    assert [j["src_type"] for j in jobs] == ["p010le"] * 2 + ["yuv420p10le"] * 2
    bad = {"root_path": "/data", "test_classes": {"X": dict(config["test_classes"]["HW"], src_type="rgb24")}}
    with pytest.raises(ValueError, match="rgb24"):
        harness.jobs_from_config(bad, {})
    seen = []
    monkeypatch.setattr(harness, "run_one_point", lambda *a, **kw: seen.append((kw["src_type"], kw["rec_path"])) or {})
    harness.run_job(("i", "p"), jobs[0], {})
    harness.run_job(("i", "p"), jobs[2], {})
    assert seen == [("p010le", None), ("yuv420p10le", None)]


def test_unknown_or_impossible_sources_are_refused_before_any_device_work():
    with pytest.raises(ValueError, match="rgb24"):
        harness.run_one_point(None, None, "/nonexistent.yuv", 64, 64, 1, 0, src_type="rgb24")
    with pytest.raises(ValueError, match="even"):
        harness.run_one_point(None, None, "/nonexistent.yuv", 63, 64, 1, 0, src_type="yuv420p10le")


# ------------------------------------------------------------------------------------------- the restatement itself
@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "frame_io_hbd.npz"))


@pytest.mark.parametrize("tag,chroma,bits", R.CASES)
def test_restatement_equals_the_reference_reader(gold, tag, chroma, bits):
    """sample / max_val in fp32 + nearest up-sampling == YUVReader.read_one_frame + ycbcr420_to_444, bit for bit; the pad
    replicates the last row / column"""
    want = gold[f"frame_{tag}_{chroma}_{bits}"]
    _, h, w = want.shape
    planes = R.fixture_source(gold, tag, chroma, bits)
    for dt in (np.float32, np.float16):
        got = R.load_ref(planes, chroma, bits, dt)
        assert got.dtype == dt and got.shape == (1, 3, h + (-h) % 16, w + (-w) % 16)
        assert np.array_equal(got[0, :, :h, :w], want.astype(dt))
        assert np.array_equal(got[0, :, h:, :], np.broadcast_to(got[0, :, h - 1:h, :], got[0, :, h:, :].shape))
        assert np.array_equal(got[0, :, :, w:], np.broadcast_to(got[0, :, :, w - 1:w], got[0, :, :, w:].shape))


@pytest.mark.parametrize("tag,chroma,bits", R.CASES)
def test_restatement_equals_the_reference_writer(gold, tag, chroma, bits):
    """((a + b) + (d + e)) * 0.25f, clip, * max_val, rint, clip == ycbcr444_to_420 + YUVWriter.write_one_frame for fp32 and
    fp16-valued reconstructions: every sample, no tolerance"""
    for name, dt in (("f32", np.float32), ("f16", np.float16)):
        x, h, w = R.fixture_reconstruction(gold, tag, dt)
        got = R.store_ref(x, h, w, chroma, bits)
        for g, want, k in zip(got, R.fixture_written(gold, tag, chroma, bits, name), "yuv"):
            assert g.dtype == np.uint16 and np.array_equal(g, want), (name, k, int((g != want).sum()))


def test_fixture_reconstruction_leaves_the_unit_interval_on_both_sides(gold):
    for tag in "abc":
        x = gold[f"rec_{tag}"]
        assert 0.005 < np.mean(x < 0) < 0.05 and 0.005 < np.mean(x > 1) < 0.05


def test_the_two_identities_of_the_contract():
    """257 * s8 / 65535 and s8 / 255 are the same fp32 (so a 16-bit file made that way gives the 8-bit file's model input),
    and the host path's torch planes are the restatement's"""
    s8 = np.arange(256, dtype=np.uint16)
    assert np.array_equal((s8 * 257).astype(np.float32) / np.float32(65535), s8.astype(np.float32) / np.float32(255))
    import torch
    rng = np.random.default_rng(4)
    for dt in (np.float32, np.float16):
        x = rng.uniform(-0.05, 1.05, (1, 3, 48, 64)).astype(np.float32).astype(dt)
        for name in ("yuv420p10le", "yuv444p12le", "p010le", "yuv444p"):
            f = PixelFormat.parse(name)
            got = harness.pixfmt_metric_planes(torch.from_numpy(x), 36, 50, f)
            for g, want in zip(got, R.metric_planes_ref(x, 36, 50, f.chroma, f.bit_depth)):
                assert g.dtype == torch.float32 and np.array_equal(g.numpy(), want)


def test_host_metrics_of_a_semi_planar_source_equal_the_planar_ones():
    """pixfmt_distortion on CPU tensors: P010 planes (interleaved, value in the top bits) against the same samples as
    yuv420p10le; a perfect reconstruction gives the cap"""
    import torch
    rng = np.random.default_rng(9)
    h, w = 176, 192                                   # (chroma planes of 88 x 96: the smallest MS-SSIM takes)
    y, u, v = (rng.integers(0, 1024, s).astype(np.uint16) for s in ((h, w), (h // 2, w // 2), (h // 2, w // 2)))
    x = torch.from_numpy(R.load_ref([y, u, v], 420, 10, np.float32))
    planar = [torch.from_numpy(p) for p in (y, u, v)]
    semi = [torch.from_numpy(y << 6), torch.from_numpy(R.interleave(u, v) << 6)]
    a = harness.pixfmt_distortion(x, planar, PixelFormat.parse("yuv420p10le"), calc_ssim=True)
    b = harness.pixfmt_distortion(x, semi, PixelFormat.parse("p010le"), calc_ssim=True)
    assert a == b and a[0] == [99.9] * 4 and all(abs(m - 1.0) < 1e-12 for m in a[1])
    noisy = (x + torch.from_numpy(rng.normal(0, 0.01, tuple(x.shape)).astype(np.float32))).half()
    a = harness.pixfmt_distortion(noisy, planar, PixelFormat.parse("yuv420p10le"))
    assert a == harness.pixfmt_distortion(noisy, semi, PixelFormat.parse("p010le")) and 30 < a[0][1] < 50 and a[1] == [0.0] * 4
