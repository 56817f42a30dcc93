"""The device resampler and reduced-resolution coding (csrc/dcvc_resize.hip, opendcvc_amd/resize.py, the container's display
unit, the harness's --coded-size) as far as a GPU-less host can check them: the tables, the numpy restatement the GPU tests
compare with against Pillow and torch, the container unit byte for byte, argument errors without a device, and the options'
way through the harness."""
import ctypes
import io
import os
import re
import types

import numpy as np
import pytest

import resize_ref as R
from opendcvc_amd import _lib, bitstream, harness, resize
from opendcvc_amd.bitstream import NalType, StreamReader, StreamWriter

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILTERS = ("bilinear", "bicubic", "lanczos3")
SHAPES = [((72, 120), (48, 80)), ((48, 80), (72, 120)), ((70, 118), (37, 51)), ((37, 51), (70, 118)), ((270, 480), (180, 320))]


# ------------------------------------------------------------------------------------------- tables
@pytest.mark.parametrize("name", FILTERS)
def test_every_row_of_a_table_sums_to_one(name):
    for n_in, n_out in ((120, 80), (80, 120), (118, 51), (51, 118), (64, 8), (8, 64), (1920, 1280), (1080, 720), (3, 24)):
        first, coef = resize.filter_taps(name, n_in, n_out)
        assert first.dtype == np.int32 and coef.dtype == np.float32 and first.shape == (n_out,) and coef.shape[0] == n_out
        last = coef.shape[1] - 1 - (coef[:, ::-1] != 0).argmax(1)                  # the last non-zero tap of every row
        assert first.min() >= 0 and (first + last).max() < n_in
        s = coef.astype(np.float64).sum(1)
        assert np.abs(s - 1.0).max() <= 2 * np.finfo(np.float32).eps, (n_in, n_out, np.abs(s - 1.0).max())


@pytest.mark.parametrize("name", FILTERS)
def test_identity_tables_and_the_abi_limit(name):
    first, coef = resize.filter_taps(name, 37, 37)
    assert np.array_equal(first, np.arange(37)) and coef.shape == (37, 1) and np.all(coef == 1.0)
    for n_in, n_out in ((64, 8), (8, 64), (800, 100), (1000, 125)):
        assert resize.filter_taps(name, n_in, n_out)[1].shape[1] <= 64
    assert 40 <= max(resize.filter_taps("lanczos3", n, n // 8)[1].shape[1] for n in (64, 800, 1000, 1096)) <= 49
    for n_in, n_out in ((801, 100), (100, 801)):
        with pytest.raises(ValueError, match="ratio"):
            resize.filter_taps(name, n_in, n_out)


def test_unknown_filter_names_are_refused():
    for name in ("nearest", "lanczos", "LANCZOS3", "", None):
        with pytest.raises(ValueError):
            resize.filter_taps(name, 16, 8)


# ------------------------------------------------------------------------------------------- the restatement
@pytest.fixture(scope="module")
def planes():
    """fp32 data uniform in [0, 1) per source size, made once, never modified"""
    rng = np.random.default_rng(12)
    data = {size: rng.random((3,) + size, dtype=np.float32) for size in {a for a, _ in SHAPES}}
    for v in data.values():
        v.setflags(write=False)
    return data


@pytest.mark.parametrize("name", FILTERS)
@pytest.mark.parametrize("size_in,size_out", SHAPES)
def test_restatement_equals_pillow(planes, size_in, size_out, name):
    Image = pytest.importorskip("PIL.Image")
    x = planes[size_in]
    got = R.resize_ref(x, size_in, size_out, name)
    how = {"bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC, "lanczos3": Image.LANCZOS}[name]
    want = np.stack([np.asarray(Image.fromarray(np.ascontiguousarray(x[c]), mode="F").resize(size_out[::-1], how)) for c in range(3)])
    d = float(np.abs(got - want).max())
    print(f"{size_in} -> {size_out} {name}: max |restatement - Pillow| = {d:.3g}")
    assert got.shape == want.shape == (3,) + size_out and d <= 1e-6


@pytest.mark.parametrize("name", ["bilinear", "bicubic"])
@pytest.mark.parametrize("size_in,size_out", SHAPES)
def test_restatement_equals_torch_antialias(planes, size_in, size_out, name):
    import torch
    x = planes[size_in]
    got = R.resize_ref(x, size_in, size_out, name)
    want = torch.nn.functional.interpolate(torch.from_numpy(np.array(x))[None], size=size_out, mode=name, antialias=True,
                                           align_corners=False)[0].numpy()
    d = float(np.abs(got - want).max())
    print(f"{size_in} -> {size_out} {name}: max |restatement - torch| = {d:.3g}")
    assert d <= 2e-5


@pytest.mark.parametrize("name", FILTERS)
def test_restatement_identity_constant_and_padding(planes, name):
    x = planes[(70, 118)]
    assert np.array_equal(R.resize_ref(x, (70, 118), (70, 118), name), x)
    half = x.astype(np.float16)
    assert np.array_equal(R.resize_ref(half, (70, 118), (70, 118), name), half)
    # a constant plane: the mid-range constant of the [0, 1] data, 0.5, for which the bound 2.4e-7 = 2^-22 is 4 ulp - each
    # of the two passes is a sum whose weights add up to 1 within 2 ulp of 1 and whose value stays near the constant.  (The
    # error grows with the constant: at 1.0 the same arithmetic is off by up to 3.6e-7 for 70x118 -> 37x51.)
    for size_in, size_out in SHAPES:
        out = R.resize_ref(np.full((3,) + size_in, 0.5, np.float32), size_in, size_out, name)
        d = float(np.abs(out - np.float32(0.5)).max())
        print(f"{size_in} -> {size_out} {name}: constant 0.5 comes back within {d:.3g}")
        assert d <= 2.4e-7
    # the source's padding is not read, the output's is the replicate pad
    big = np.full((3, 80, 128), np.nan, np.float32)
    big[:, :70, :118] = x
    out = R.resize_ref(big, (70, 118), (37, 51), name, pad_to=16)
    assert out.shape == (3, 48, 64) and np.isfinite(out).all()
    assert np.array_equal(out[:, :37, :51], R.resize_ref(x, (70, 118), (37, 51), name))
    assert np.array_equal(out[:, 37:, :], np.broadcast_to(out[:, 36:37, :], out[:, 37:, :].shape))
    assert np.array_equal(out[:, :, 51:], np.broadcast_to(out[:, :, 50:51], out[:, :, 51:].shape))


# ------------------------------------------------------------------------------------------- container
def _pkt(is_i, payload=b"\x01\x02\x03", digest=None):
    return types.SimpleNamespace(is_i=is_i, qp=7, use_ada_i=0, bit_stream=payload, digest=digest, chunked=False)


def _by_hand(frames, height, width):
    """the stream of today: an SPS in front of the first frame, then write_ip per frame"""
    out = io.BytesIO()
    bitstream.write_sps(out, dict(sps_id=0, height=height, width=width, ec_part=0, use_ada_i=0))
    for p in frames:
        bitstream.write_ip(out, p.is_i, 0, p.qp, p.bit_stream)
    return out.getvalue()


def test_display_unit_layout_and_round_trip():
    assert int(NalType.NAL_DISPLAY) == 6
    out = io.BytesIO()
    assert bitstream.write_display(out, 3, 1080, 1920, "lanczos3") == 6
    assert out.getvalue() == bytes((0x63, 0x80 | (1080 >> 8), 1080 & 0xff, 0x80 | (1920 >> 8), 1920 & 0xff, 2))
    out = io.BytesIO()
    assert bitstream.write_display(out, 0, 96, 100, "bilinear") == 4 and out.getvalue() == bytes((0x60, 96, 100, 0))
    for fid, name in enumerate(FILTERS):
        out = io.BytesIO()
        bitstream.write_display(out, 1, 2160, 3840, name)
        f = io.BytesIO(out.getvalue())
        head = bitstream.read_header(f)
        assert head == {"nal_type": NalType.NAL_DISPLAY, "sps_id": 1} and out.getvalue()[-1] == fid
        assert bitstream.read_display_remaining(f) == (2160, 3840, name)
    with pytest.raises(ValueError):
        bitstream.write_display(io.BytesIO(), 0, 96, 128, "nearest")


def test_writer_puts_the_unit_behind_every_sps_and_in_front_of_a_digest():
    out = io.BytesIO()
    w = StreamWriter(out, display=(96, 128, "bicubic"))
    frames = [_pkt(True, digest=0x1122334455667788), _pkt(False, digest=5)]
    sizes = [w.write_frame(64, 80, False, p) for p in frames]
    # a second SPS (the entropy-coder split changes): the unit is written again, under the new id
    sizes.append(w.write_frame(64, 80, True, _pkt(True, digest=6)))
    data = out.getvalue()
    assert sum(sizes) == len(data)
    sps0, disp0 = bytes((0x00, 64, 80, 0)), bytes((0x60, 96, 0x80, 128, 1))
    assert data.startswith(sps0 + disp0 + bytes((0x50,)) + (0x1122334455667788).to_bytes(8, "little") + bytes((0x10, 7, 3, 1, 2, 3)))
    assert sizes[0] == 4 + 5 + 9 + 6 and sizes[1] == 9 + 6 and sizes[2] == 4 + 5 + 9 + 6
    assert data[sizes[0] + sizes[1]:].startswith(bytes((0x01, 64, 80, 4)) + bytes((0x61, 96, 0x80, 128, 1)) + bytes((0x51,)))
    r = StreamReader(io.BytesIO(data))
    assert r.display is None
    for k in range(3):
        sps, is_i, qp, payload = r.read_frame()
        assert (sps["height"], sps["width"], sps["sps_id"]) == (64, 80, 0 if k < 2 else 1) and payload == b"\x01\x02\x03"
        assert r.display == (96, 128, "bicubic") and r.digest == (0x1122334455667788, 5, 6)[k]
    with pytest.raises(EOFError):
        r.read_frame()


def test_streams_without_scaling_are_the_bytes_of_today():
    frames = [_pkt(True), _pkt(False), _pkt(False)]
    want = _by_hand(frames, 64, 80)
    for display in (None, (64, 80, "lanczos3")):
        out = io.BytesIO()
        w = StreamWriter(out, display=display)
        sizes = [w.write_frame(64, 80, False, p) for p in frames]
        assert out.getvalue() == want and sum(sizes) == len(want)
        r = StreamReader(io.BytesIO(out.getvalue()))
        for _ in frames:
            r.read_frame()
            assert r.display is None
    plain = io.BytesIO()
    w = StreamWriter(plain)
    for p in frames:
        w.write_frame(64, 80, False, p)
    assert plain.getvalue() == want


def test_damaged_display_units_raise():
    sps = bytes((0x00, 64, 80, 0))
    frame = bytes((0x10, 7, 1, 9))
    ok = sps + bytes((0x60, 96, 0x80, 128, 2)) + frame
    r = StreamReader(io.BytesIO(ok))
    r.read_frame()
    assert r.display == (96, 128, "lanczos3")
    for cut in range(len(sps) + 1, len(sps) + 5):           # the unit ends after its header, inside a varint, before the filter id
        with pytest.raises(EOFError):
            StreamReader(io.BytesIO(ok[:cut])).read_frame()
    with pytest.raises(ValueError, match="filter id 3"):
        StreamReader(io.BytesIO(sps + bytes((0x60, 96, 0x80, 128, 3)) + frame)).read_frame()
    for disp in (bytes((0x60, 63, 0x80, 128, 2)), bytes((0x60, 96, 79, 2))):       # below the coded size in one dimension
        with pytest.raises(ValueError, match="below"):
            StreamReader(io.BytesIO(sps + disp + frame)).read_frame()
    with pytest.raises(ValueError, match="unknown SPS"):
        StreamReader(io.BytesIO(bytes((0x62, 96, 0x80, 128, 2)) + frame)).read_frame()
    with pytest.raises(ValueError, match="below"):
        StreamWriter(io.BytesIO(), display=(96, 64, "bilinear")).write_frame(64, 80, False, _pkt(True))
    with pytest.raises(ValueError):
        StreamWriter(io.BytesIO(), display=(96, 128, "nearest"))


# ------------------------------------------------------------------------------------------- the C entry
def test_entry_is_declared_bound_and_exported():
    header = open(os.path.join(REPO, "include", "dcvc_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert os.path.exists(_lib.LIB_PATH), "libdcvc_amd.so not built (run __graft_entry__.build())"
    assert re.search(r"\bdcvc_resize_frame\s*\(", code) and "dcvc_resize_frame" in _lib.EXPORTS
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "dcvc_resize_frame")
    assert re.search(r"#define\s+DCVC_ABI_VERSION\s+1\b", header) and _lib.lib().dcvc_abi_version() == 1


# a 64-byte-aligned host buffer stands in for every pointer: each call below must be refused before anything is launched
_BUF = ctypes.create_string_buffer(4096 + 64)
_PTR = (ctypes.addressof(_BUF) + 63) & ~63


def _resize(dtype=_lib.F16, x=_PTR, Hp=32, Wp=48, H=30, W=40, out=_PTR, HOp=16, WOp=32, HO=15, WO=20, fh=_PTR, ch=_PTR, th=6,
            fv=_PTR, cv=_PTR, tv=6):
    return _lib.lib().dcvc_resize_frame(dtype, x, Hp, Wp, H, W, out, HOp, WOp, HO, WO, fh, ch, th, fv, cv, tv, None)


def test_argument_errors_need_no_device():
    bad = [dict(dtype=_lib.U8), dict(dtype=-1),
           dict(H=0), dict(W=0), dict(HO=0), dict(WO=-1), dict(Hp=29), dict(Wp=39), dict(HOp=14), dict(WOp=16),
           dict(th=0), dict(th=65), dict(tv=0), dict(tv=65),
           dict(x=None), dict(out=None), dict(fh=None), dict(ch=None), dict(fv=None), dict(cv=None),
           dict(x=_PTR + 1), dict(dtype=_lib.F32, x=_PTR + 2), dict(out=_PTR + 8), dict(WOp=28), dict(WOp=36),
           dict(fh=_PTR + 2), dict(ch=_PTR + 1), dict(fv=_PTR + 2), dict(cv=_PTR + 2)]
    before = bytes(_BUF)
    for kw in bad:
        assert _resize(**kw) == -1, kw
        assert b"dcvc_resize_frame" in _lib.lib().dcvc_last_error(), kw
    assert bytes(_BUF) == before


# ------------------------------------------------------------------------------------------- harness plumbing
def test_coded_size_parses_and_reaches_the_jobs_and_run_one_point(monkeypatch):
    ap = harness.build_parser()
    base = "--src a.yuv --width 1920 --height 1080 --frames 1"
    for opt in ("--coded-size", "--coded_size"):
        assert ap.parse_args(f"{base} {opt} 1280x720".split()).coded_size == (720, 1280)
    args = ap.parse_args(base.split())
    assert args.coded_size is None and args.scale_filter == "lanczos3"
    for opt in ("--scale-filter", "--scale_filter"):
        for name in FILTERS:
            assert ap.parse_args(f"{base} {opt} {name}".split()).scale_filter == name
    for text in ("--coded-size 1280", "--coded-size 1280x", "--coded-size 1280x720x3", "--coded-size axb", "--coded-size -1280x720",
                 "--scale-filter nearest"):
        with pytest.raises(SystemExit):
            ap.parse_args(f"{base} {text}".split())
    args = ap.parse_args("--test-config m.json --coded-size 1280x720 --scale-filter bicubic".split())
    opts, _ = harness.manifest_options(args, ap)
    assert opts["coded_size"] == (720, 1280) and opts["scale_filter"] == "bicubic"
    config = {"root_path": "/data", "test_classes": {"HW": {"test": 1, "base_path": "hw", "src_type": "yuv420", "sequences": {
        "a.yuv": {"width": 1920, "height": 1080, "frames": 2, "intra_period": -1}}}}}
    jobs = harness.jobs_from_config(config, dict(opts, qp_i=[10]))
    seen = []
    monkeypatch.setattr(harness, "run_one_point", lambda *a, **kw: seen.append((kw["coded_size"], kw["scale_filter"])) or {})
    harness.run_job(("i", "p"), jobs[0], opts)
    harness.run_job(("i", "p"), jobs[0], {})
    assert seen == [((720, 1280), "bicubic"), (None, "lanczos3")]
    # the single-sequence command line hands both on too
    swept = []
    monkeypatch.setattr(harness, "run_sweep", lambda *a, **kw: swept.append((kw["coded_size"], kw["scale_filter"])) or {})
    harness.main(f"{base} --coded-size 960x540 --scale-filter bilinear --out {os.devnull}".split())
    assert swept == [((540, 960), "bilinear")]


def test_impossible_coded_sizes_are_refused_before_any_device_work():
    run = lambda **kw: harness.run_one_point(None, None, "/nonexistent.yuv", 128, 96, 1, 0, **kw)
    for size, what in (((97, 128), "above"), ((96, 129), "above"), ((15, 128), "at least 16"), ((96, 8), "at least 16")):
        with pytest.raises(ValueError, match=what):
            run(coded_size=size)
    with pytest.raises(ValueError, match="nearest"):
        run(coded_size=(64, 80), scale_filter="nearest")
    with pytest.raises(ValueError, match="WIDTHxHEIGHT"):
        resize.parse_size("1280*720")
    assert resize.check_coded_size(None, 96, 128) is None and resize.check_coded_size((96, 128), 96, 128) is None
    assert resize.check_coded_size((64, 80), 96, 128) == (64, 80)
