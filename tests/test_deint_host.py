"""Deinterlacing without a device (docs/deinterlace.md): the properties of the numpy restatement (tests/deint_ref.py) the
document states, both decision rules on clips whose class is known, every argument error of the two C entries, the harness's
options, and the front end and the decode pass's reference-picture rule on stubs."""
import ctypes
import inspect
import os

import numpy as np
import pytest

import deint_ref as R
from opendcvc_amd import _lib, deinterlace, harness

F16_32 = [pytest.param(np.float32, id="fp32"), pytest.param(np.float16, id="fp16")]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint16 if a.dtype == np.float16 else np.uint32)


def _noise(ndt, H, W, seed):
    return np.random.default_rng(seed).random((3, H, W), dtype=np.float32).astype(ndt)


# ---------------------------------------------------------------------------------- the restatement's properties
@pytest.mark.parametrize("ndt", F16_32)
@pytest.mark.parametrize("lines", [1, 2])
@pytest.mark.parametrize("parity", [0, 1])
def test_kept_rows_are_bit_copies_whatever_they_hold(parity, lines, ndt):
    H, W = 24, 20
    cur, prev = _noise(ndt, H, W, 1), _noise(ndt, H, W, 2)
    cur[0, 2 + parity, 3], cur[1, 4 * 1 + 2 * parity, 5] = np.nan, np.inf            # on kept rows (luma; chroma where lines == 2)
    for p in (None, prev):
        out = R.deinterlace(cur, p, H, W, parity, lines)
        assert out.dtype == ndt and out.shape == cur.shape
        for plane, L in ((0, 1), (1, lines), (2, lines)):
            kept = [y for y in range(H) if (y // L) % 2 == parity]
            missing = R.missing_rows(H, parity, L)
            assert sorted(kept + missing) == list(range(H)) and len(kept) == len(missing) == H // 2
            assert np.array_equal(_bits(out[plane, kept]), _bits(cur[plane, kept]))
            assert not np.array_equal(_bits(out[plane, missing]), _bits(cur[plane, missing]))


@pytest.mark.parametrize("ndt", F16_32)
def test_a_static_monotone_picture_comes_out_bit_for_bit(ndt):
    H, W = 32, 24
    for sign in (1.0, -1.0):
        ramp = np.cumsum(np.random.default_rng(3).random((3, H, W)), axis=1)
        ramp = (ramp / ramp.max())[:, ::int(sign)].astype(ndt)                  # monotone along every column, up or down
        for lines in (1, 2):
            x = ramp.copy()
            if lines == 2:
                x[1:] = np.repeat(x[1:, ::2], 2, 1)                             # rows in pairs: still monotone (not strictly)
            for parity in (0, 1):
                assert np.array_equal(_bits(R.deinterlace(x, x, H, W, parity, lines)), _bits(x))


@pytest.mark.parametrize("ndt", F16_32)
def test_a_static_picture_of_alternating_lines_is_flattened(ndt):
    H, W = 16, 12
    comb = np.zeros((3, H, W), ndt)
    comb[:, 0::2], comb[:, 1::2] = 0.25, 0.75
    assert (R.deinterlace(comb, comb, H, W, 0, 1) == ndt(0.25)).all()           # the known limit: it cannot be told from a comb
    assert (R.deinterlace(comb, comb, H, W, 1, 1) == ndt(0.75)).all()


@pytest.mark.parametrize("ndt", F16_32)
def test_without_a_previous_frame_the_predictor_is_spatial_only(ndt):
    H, W = 8, 16
    # rows that are flat: every direction scores 0, the straight one is preferred, the mean of the lines above and below
    x = np.repeat(np.arange(H, dtype=np.float32)[:, None] / 16, W, 1)[None].repeat(3, 0).astype(ndt)
    out = R.deinterlace(x, None, H, W, 0, 1)
    for y in (1, 3, 5):
        assert (out[:, y] == ndt((np.float32(x[0, y - 1, 0]) + np.float32(x[0, y + 1, 0])) * np.float32(0.5))).all()
    assert (out[:, 7] == x[:, 6]).all()                                         # the last line: +1 leaves, -1 is taken twice
    # a diagonal edge, one column per line: the direction along the edge wins and the edge stays sharp
    edge = np.zeros((3, H, W), ndt)
    for y in range(H):
        edge[:, y, :4 + y] = 1.0
    out = R.deinterlace(edge, None, H, W, 0, 1)
    assert set(np.unique(out[:, 3]).tolist()) == {0.0, 1.0} and np.array_equal(out[:, 3], edge[:, 3])
    # what a previous frame says is not looked at, and after a change of shape there is none
    d = R.Deinterlacer("on", "tff", 1)
    a, b = _noise(ndt, H, W, 5), _noise(ndt, H, W, 6)
    assert np.array_equal(d.filter(a, (H, W)), R.deinterlace(a, None, H, W, 0, 1))
    assert np.array_equal(d.filter(b, (H, W)), R.deinterlace(b, a, H, W, 0, 1))
    assert not np.array_equal(R.deinterlace(b, a, H, W, 0, 1), R.deinterlace(b, None, H, W, 0, 1))
    assert np.array_equal(d.filter(x, (H - 2, W)), R.deinterlace(x, None, H - 2, W, 0, 1))
    d.reset()
    assert np.array_equal(d.filter(x, (H - 2, W)), R.deinterlace(x, None, H - 2, W, 0, 1))
    with pytest.raises(ValueError):
        R.deinterlace(x, None, 6, W, 0, 2)


def _mse(lines, speed, ndt, parity):
    """MSE in squared 8-bit codes against the true progressive frames of a moving interlaced clip, [luma, chroma] x (weave,
    spatial only, the filter)"""
    H, W, n = 64, 96, 4
    clip, truth = R.make_clip("interlaced", n, H, W, speed=speed, seed=speed, parity=parity, chroma_lines=lines)
    order = "tff" if parity == 0 else "bff"
    full, alone = R.Deinterlacer("on", order, lines), R.Deinterlacer("on", order, lines)
    err = np.zeros((2, 3))
    for planes, true in zip(clip, truth):
        x, t = R.to_frame(planes, ndt), R.to_frame(true, ndt).astype(np.float64)
        alone.reset()
        for k, y in enumerate((x, alone.filter(x, (H, W)), full.filter(x, (H, W)))):
            e = (y.astype(np.float64) - t) ** 2 * 255.0 ** 2 / n
            err[0, k] += np.mean(e[0])
            err[1, k] += np.mean(e[1:])
    return err


@pytest.mark.parametrize("ndt", F16_32)
@pytest.mark.parametrize("lines,parity", [(1, 0), (2, 0), (2, 1)])
def test_on_a_moving_interlaced_clip_the_filter_is_closer_to_the_truth_than_weaving(lines, parity, ndt):
    """speed: pixels per frame.  Luma and 4:4:4 chroma: below weaving at every speed, and at or below the spatial predictor
    alone up to two pixels per frame.  The chroma of 4:2:0 has lines two rows high and is rebuilt from rows four apart: it is
    below weaving from two pixels per frame on; at one pixel per frame - half a pixel per field - the weave of so smooth a
    texture is nearer the truth (docs/deinterlace.md states it)"""
    for speed in (1, 2, 4):
        err = _mse(lines, speed, ndt, parity)
        for name, (weave, spatial, both) in zip(("luma", "chroma"), err):
            print(f"chroma_lines {lines} parity {parity} speed {speed} {name}: weave {weave:.2f} spatial {spatial:.2f} filter {both:.2f}")
            if name == "luma" or lines == 1 or speed >= 2:
                assert both < weave, (name, speed)
            if speed <= 2:
                assert both <= spatial, (name, speed)                           # slow motion: the previous frame helps


# ---------------------------------------------------------------------------------- the decision rules
H0, W0 = 96, 128


def _ratios(kind, speed, vy=0, sigma=0.0, blur=2, parity=0):
    clip, _ = R.make_clip(kind, 3, H0, W0, speed=speed, vy=vy, sigma=sigma, seed=speed + 7 * vy, parity=parity, blur=blur)
    fr = [R.to_frame(f) for f in clip]
    with_prev = []
    for t in (1, 2):
        dc, dp = R.comb_sums(fr[t], fr[t - 1], H0, W0, parity)
        assert R.comb_decision(fr[t], fr[t - 1], H0, W0, parity) == (0 if 8 * dc < 7 * dp else 1)
        with_prev.append(dc / dp)
    dc, ds = R.comb_sums(fr[0], None, H0, W0, parity)
    assert R.comb_decision(fr[0], None, H0, W0, parity) == (1 if dc > ds else 0)
    return with_prev, dc / ds


@pytest.mark.parametrize("parity", [0, 1])
@pytest.mark.parametrize("blur", [1, 2])
def test_both_rules_on_clips_whose_class_is_known(blur, parity):
    """the margins are those of the document's table: progressive material that moves stays below 0.5 of the 0.875 threshold,
    interlaced and static material within 0.05 of 1; without a previous frame progressive stays below 0.7 and interlaced
    material moving two pixels per frame or more above 1.2"""
    for sigma in (0.0, 4.0):
        for vy in (0, 1):
            for speed in (1, 2, 4, 8):
                prog, first = _ratios("progressive", speed, vy, sigma, blur, parity)
                assert max(prog) < 0.5 and first < 0.7, (speed, vy, sigma, prog, first)
                inter, first = _ratios("interlaced", speed, vy, sigma, blur, parity)
                assert 0.95 < min(inter) and max(inter) < 1.05, (speed, vy, sigma, inter)
                assert first > 1.2 or speed < 2, (speed, vy, sigma, first)
        static, first = _ratios("static", 1, 0, sigma, blur, parity)
        assert 0.95 < min(static) and max(static) < 1.05 and first < 0.7
    # the stated limit of the rule without a previous frame: one line per field straight up looks like a progressive frame
    clip, _ = R.make_clip("interlaced", 1, H0, W0, speed=0, vy=1, seed=2, parity=parity, blur=blur)
    x = R.to_frame(clip[0])
    assert R.comb_decision(x, None, H0, W0, parity) == 0


def test_the_sums_are_64_bit_and_the_quantiser_is_the_temporal_filters():
    import tf_ref
    v = np.array([-1.0, 0.0, 0.5, 1.0, 2.0, np.nan, 0.25 + 1 / 2046], np.float32)
    assert np.array_equal(R.quant(v), tf_ref.quant(v).astype(np.int64))
    H, W = 2162, 3840                                      # a 4K plane of the worst comb: above 32 bits
    x = np.zeros((3, H, W), np.float16)
    x[0, 1::2] = 1.0
    dc, ds = R.comb_sums(x, None, H, W, 0)
    assert dc == 2046 * (H // 2 - 1) * W > 1 << 32 and ds == 0


# ---------------------------------------------------------------------------------- the C entries' argument errors
# a 64-byte-aligned host buffer stands in for every pointer: each call below must be refused before anything is launched
_BUF = ctypes.create_string_buffer(4 * 24576 + 256)
_PTR = (ctypes.addressof(_BUF) + 63) & ~63
_CUR, _PREV, _OUT, _WS = _PTR, _PTR + 24576, _PTR + 2 * 24576, _PTR + 3 * 24576          # frames of 3 * 32 * 48 fp32 elements: 18432 bytes
_WORD = _WS + 64


def _deint(dtype=_lib.F16, cur=_CUR, prev=_PREV, Hp=32, Wp=48, H=28, W=40, parity=0, lines=2, decision=_WORD, out=_OUT):
    return _lib.lib().dcvc_deinterlace(dtype, cur, prev, Hp, Wp, H, W, parity, lines, decision, out, None)


def _comb(dtype=_lib.F16, cur=_CUR, prev=_PREV, Hp=32, Wp=48, H=28, W=40, parity=0, ws=_WS, decision=_WORD):
    return _lib.lib().dcvc_comb_detect(dtype, cur, prev, Hp, Wp, H, W, parity, ws, decision, None)


BAD_FRAME = [dict(dtype=_lib.U8), dict(dtype=-1), dict(cur=None), dict(cur=_CUR + 1), dict(prev=_PREV + 1), dict(H=0), dict(W=0),
             dict(H=-4), dict(W=-1), dict(Hp=8), dict(Wp=8), dict(Hp=1 << 20, Wp=1 << 20), dict(parity=2), dict(parity=-1),
             dict(dtype=_lib.F32, cur=_CUR + 2), dict(dtype=_lib.F32, prev=_PREV + 2), dict(decision=_WORD + 2)]
BAD_DEINT = BAD_FRAME + [dict(out=None), dict(out=_OUT + 1), dict(dtype=_lib.F32, out=_OUT + 2), dict(lines=0), dict(lines=3), dict(lines=4),
                         dict(H=27), dict(H=26), dict(H=30, lines=2), dict(H=27, lines=1), dict(out=_CUR), dict(out=_PREV),
                         dict(out=_CUR + 9216 - 2), dict(out=_PREV - 9216 + 2), dict(dtype=_lib.F32, out=_CUR + 18428),
                         dict(prev=None, out=_CUR)]
BAD_COMB = BAD_FRAME + [dict(ws=None), dict(ws=_WS + 4), dict(decision=None), dict(H=27), dict(H=1)]


@pytest.mark.parametrize("kw", BAD_DEINT, ids=lambda kw: "-".join(kw))
def test_deinterlace_refuses_a_bad_argument_by_name_before_any_launch(kw):
    before = bytes(_BUF)
    assert _deint(**kw) == -1, kw
    err = _lib.lib().dcvc_last_error()
    assert b"dcvc_deinterlace" in err, err
    assert bytes(_BUF) == before


@pytest.mark.parametrize("kw", BAD_COMB, ids=lambda kw: "-".join(kw))
def test_comb_detect_refuses_a_bad_argument_by_name_before_any_launch(kw):
    before = bytes(_BUF)
    assert _comb(**kw) == -1, kw
    err = _lib.lib().dcvc_last_error()
    assert b"dcvc_comb_detect" in err, err
    assert bytes(_BUF) == before


def test_the_messages_name_what_is_wrong_and_the_exports_are_there():
    L = _lib.lib()
    for call, kw, word in ((_deint, dict(H=26), b"multiple of 4"), (_deint, dict(H=27, lines=1), b"multiple of 2"),
                           (_deint, dict(lines=3), b"chroma_lines"), (_deint, dict(parity=2), b"keep_parity"),
                           (_deint, dict(out=_CUR), b"overlaps the current"), (_deint, dict(out=_PREV), b"overlaps the previous"),
                           (_deint, dict(Hp=8), b"does not hold the picture"), (_deint, dict(out=None), b"null"),
                           (_comb, dict(ws=None), b"workspace"), (_comb, dict(decision=None), b"decision"), (_comb, dict(H=27), b"even")):
        assert call(**kw) == -1 and word in L.dcvc_last_error(), (kw, L.dcvc_last_error())
    assert L.dcvc_comb_ws_bytes() == 64
    for name in ("dcvc_deinterlace", "dcvc_comb_detect", "dcvc_comb_ws_bytes"):
        assert name in _lib.EXPORTS and hasattr(L, name)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    make = open(os.path.join(root, "opendcvc_amd", "csrc", "Makefile")).read()
    assert make.count("dcvc_deint.o") >= 3 and "dcvc_deint.o: CXXFLAGS += -mllvm -amdgpu-kernarg-preload-count=2" in make


# ---------------------------------------------------------------------------------- the options
BASE = "--src a.yuv --width 64 --height 64 --frames 1".split()


def test_check_deinterlace_and_check_height():
    assert deinterlace.check_deinterlace(None) == (None, 0) == deinterlace.check_deinterlace(None, "tff")
    assert deinterlace.check_deinterlace("on") == ("on", 0) and deinterlace.check_deinterlace("auto", "bff") == ("auto", 1)
    for mode, order, word in (("off", "tff", "deinterlace"), (True, "tff", "deinterlace"), ("on", "top", "field_order"),
                              ("auto", None, "field_order"), (None, "bff", "field_order"), (None, "x", "field_order")):
        with pytest.raises(ValueError, match=word):
            deinterlace.check_deinterlace(mode, order)
    deinterlace.check_height(1080, 1)
    deinterlace.check_height(1080, 2)
    for height, lines in ((1082, 2), (1081, 1), (0, 1), (-4, 2), (8, 3)):
        with pytest.raises(ValueError):
            deinterlace.check_height(height, lines)


def test_deint_kwargs_and_the_parser_spellings():
    assert harness.deint_kwargs({}) == {} == harness.deint_kwargs(dict(deinterlace=None, field_order=None))
    assert harness.deint_kwargs(dict(deinterlace=None, field_order="bff")) == {}
    assert harness.deint_kwargs(dict(deinterlace="on", field_order=None, other=1)) == {"deinterlace": "on"}
    assert harness.deint_kwargs(dict(deinterlace="auto", field_order="bff")) == {"deinterlace": "auto", "field_order": "bff"}
    ap = harness.build_parser()
    assert ap.get_default("deinterlace") is None and ap.get_default("field_order") is None
    assert harness.deint_kwargs(vars(ap.parse_args(BASE))) == {}
    assert harness.deint_kwargs(vars(ap.parse_args(BASE + "--deinterlace on".split()))) == {"deinterlace": "on"}
    assert harness.deint_kwargs(vars(ap.parse_args(BASE + "--deinterlace auto --field_order bff".split()))) == \
        {"deinterlace": "auto", "field_order": "bff"}
    for bad in ("--deinterlace", "--deinterlace yes", "--deinterlace on --field-order top"):
        with pytest.raises(SystemExit):
            ap.parse_args(BASE + bad.split())
    opts, _ = harness.manifest_options(ap.parse_args("--test-config m.json --gpus 1 --gpu-ids 0 --deinterlace auto --field-order tff".split()), ap)
    assert opts["deinterlace"] == "auto" and opts["field_order"] == "tff"
    opts, _ = harness.manifest_options(ap.parse_args("--test-config m.json --gpus 1 --gpu-ids 0".split()), ap)
    assert "deinterlace" not in opts and "field_order" not in opts
    params = inspect.signature(harness.run_one_point).parameters
    assert params["deinterlace"].default is None and params["field_order"].default == "tff"
    assert list(params)[-2:] == ["deinterlace", "field_order"]
    assert inspect.signature(harness._encode_pass).parameters["deint"].default is None
    assert inspect.signature(harness._decode_pass).parameters["deint"].default is None
    assert [n for n, _, _ in harness.POINT_OPTIONS][-1] == "film_grain"               # the table is not where it travels


def test_field_order_without_deinterlace_is_a_usage_error(monkeypatch):
    monkeypatch.setattr(harness, "run_sweep", lambda *a, **kw: {})
    base = BASE + ["--out", os.devnull]
    harness.main(base + "--deinterlace on --field-order bff".split())
    harness.main(base + "--deinterlace auto".split())
    for extra in ("--field-order bff", "--field-order tff"):
        with pytest.raises(SystemExit):
            harness.main(base + extra.split())


def test_without_deinterlace_run_one_point_gets_no_new_keyword(monkeypatch):
    seen = []
    monkeypatch.setattr(harness, "run_one_point", lambda *a, **kw: seen.append(kw) or {})
    monkeypatch.setattr(harness, "run_sweep", lambda *a, **kw: seen.append(kw) or {})
    job = dict(src_path="x.yuv", src_width=64, src_height=64, frame_num=2, qp_i=32, qp_p=32, intra_period=-1, reset_interval=32)
    base = BASE + ["--out", os.devnull]
    harness.run_job(("i", "p"), job, {})
    harness.main(base)
    harness.run_job(("i", "p"), job, {"deinterlace": "auto", "field_order": "bff"})
    harness.main(base + ["--deinterlace", "on"])
    for kw in seen[:2]:
        assert "deinterlace" not in kw and "field_order" not in kw
    assert (seen[2]["deinterlace"], seen[2]["field_order"]) == ("auto", "bff")
    assert seen[3]["deinterlace"] == "on" and "field_order" not in seen[3]


class _Stop(Exception):
    pass


class _Net:
    rate_estimate = entropy = None

    def set_use_two_entropy_coders(self, two):
        pass


def test_every_argument_error_comes_before_a_net_a_file_or_the_device(tmp_path, monkeypatch):
    missing = str(tmp_path / "missing.yuv")
    for kw in (dict(deinterlace="yes"), dict(deinterlace="on", field_order="top"), dict(field_order="bff"),
               dict(deinterlace="on", height=66), dict(deinterlace="auto", height=66, src_type="nv12"),
               dict(deinterlace="on", height=66, src_type="yuv420p10le"), dict(deinterlace="on", height=65, src_type="yuv444p"),
               dict(deinterlace="on", height=65, src_type="png")):
        kw = dict(kw)
        height = kw.pop("height", 64)
        with pytest.raises(ValueError):
            harness.run_one_point(None, None, missing, 64, height, 2, 32, **kw)
    # the height rule follows the source's chroma: 66 rows are two fields of whole lines in 4:4:4 and RGB, not in 4:2:0
    made, seen = [], []

    class Stub:
        def __init__(self, *a):
            made.append(a[1:])

    def encode_pass(*a, **kw):
        seen.append(kw)
        raise _Stop

    monkeypatch.setattr(deinterlace, "Deinterlacer", Stub)
    monkeypatch.setattr(harness, "_encode_pass", encode_pass)
    for src_type, lines in (("yuv444p", 1), ("png", 1), ("yuv444p10le", 1)):
        with pytest.raises(_Stop):
            harness.run_one_point(_Net(), _Net(), missing, 64, 66, 2, 32, src_type=src_type, deinterlace="auto", field_order="bff")
        assert made[-2:] == [("auto", "bff", lines)] * 2                       # one for each pass
        assert isinstance(seen[-1]["deint"], Stub)
    with pytest.raises(_Stop):
        harness.run_one_point(_Net(), _Net(), missing, 64, 64, 2, 32, deinterlace="on")
    assert made[-2:] == [("on", "tff", 2)] * 2 and len(made) == 8
    for kw in (dict(deinterlace=None), {}):                                     # off: the call of before the option, nothing is made
        with pytest.raises(_Stop):
            harness.run_one_point(_Net(), _Net(), missing, 64, 64, 2, 32, **kw)
        assert seen[-1] == {} and len(made) == 8


def test_the_source_object_knows_its_chroma_lines():
    for src_type, lines in (("yuv420", 2), ("png", 1), ("yuv420p10le", 2), ("yuv420p16le", 2), ("nv12", 2), ("p010le", 2),
                            ("yuv444p", 1), ("yuv444p12le", 1)):
        assert harness.make_source(src_type, "nowhere", 64, 64).chroma_lines == lines, src_type
    assert set(harness.SRC_TYPES) == {"yuv420", "png", "yuv420p10le", "yuv420p12le", "yuv420p16le", "yuv444p", "yuv444p10le",
                                      "yuv444p12le", "yuv444p16le", "nv12", "p010le"}


# ---------------------------------------------------------------------------------- the passes on stubs
class _Src:
    h, w, chroma_lines = 64, 96, 2

    def __init__(self, log):
        self.log = log

    def to_input(self, planes, dtype):
        self.log.append(("load", planes, dtype))
        return ("x", planes)

    def stored(self, x):
        self.log.append(("stored", x))
        return ["planes of", x]


class _Deint:
    def __init__(self, log):
        self.log = log

    def filter(self, x, size):
        self.log.append(("filter", x, size))
        return ("deinterlaced", x)


def test_the_filter_sees_every_frame_before_the_window(monkeypatch):
    from opendcvc_amd import bars
    log = []
    monkeypatch.setattr(bars, "window", lambda x, size, area: log.append(("window", x, size, area)) or ("windowed", x))
    src, di = _Src(log), _Deint(log)
    assert harness._front_input(src, "p0", "dt") == ("x", "p0")
    assert harness._front_input(src, "p1", "dt", None, "area") == ("windowed", ("x", "p1"))
    assert harness._front_input(src, "p2", "dt", di) == ("deinterlaced", ("x", "p2"))
    assert harness._front_input(src, "p3", "dt", di, "area") == ("windowed", ("deinterlaced", ("x", "p3")))
    assert log == [("load", "p0", "dt"),
                   ("load", "p1", "dt"), ("window", ("x", "p1"), (64, 96), "area"),
                   ("load", "p2", "dt"), ("filter", ("x", "p2"), (64, 96)),
                   ("load", "p3", "dt"), ("filter", ("x", "p3"), (64, 96)),             # the FULL frame, at the source's size
                   ("window", ("deinterlaced", ("x", "p3")), (64, 96), "area")]


def test_the_encode_pass_feeds_the_front_end_the_filtered_frames_in_order(monkeypatch):
    """harness._encode_pass on stubs: every frame goes reader -> loader -> Deinterlacer.filter -> FrontEnd.feed, in source order"""
    import torch
    from opendcvc_amd import frontend
    log, fed = [], []

    class Reader:
        n = 0

        def read(self):
            Reader.n += 1
            return [Reader.n]

        def close(self):
            log.append("close")

    class Front:
        units = []

        def __init__(self, *a):
            pass

        def feed(self, x, t0):
            fed.append(x)

        def flush(self):
            log.append("flush")

    class Enc:
        scenecut = None

        def __init__(self, *a, **kw):
            pass

    class P:
        def parameters(self):
            return iter([torch.zeros(1, dtype=torch.float16)])

    src = _Src(log)
    src.reader = lambda: Reader()
    monkeypatch.setattr(frontend, "FrontEnd", Front)
    monkeypatch.setattr(harness, "SequenceEncoder", Enc)
    monkeypatch.setattr(harness, "StreamWriter", lambda *a, **kw: None)
    monkeypatch.setattr(harness, "_to_device", lambda planes, dev: planes[0])
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a: None)
    done = harness._encode_pass((None, P()), src, 3, "dev", None, "lanczos3", None, {}, deint=_Deint(log))
    assert fed == [("deinterlaced", ("x", k)) for k in (1, 2, 3)] and done.repeated is None
    assert log == [("load", 1, torch.float16), ("filter", ("x", 1), (64, 96)), ("load", 2, torch.float16), ("filter", ("x", 2), (64, 96)),
                   ("load", 3, torch.float16), ("filter", ("x", 3), (64, 96)), "flush", "close"]


def test_the_decode_pass_measures_against_the_stored_deinterlaced_picture():
    log = []
    src = _Src(log)
    assert harness._reference_planes(src, "p0", "dt") == "p0" and harness._reference_planes(src, "p0", None, None) == "p0"
    assert log == []                                       # off: the source's own planes, nothing is called
    di = _Deint(log)
    assert harness._reference_planes(src, "p1", "dt", di) == ["planes of", ("deinterlaced", ("x", "p1"))]
    assert log == [("load", "p1", "dt"), ("filter", ("x", "p1"), (64, 96)), ("stored", ("deinterlaced", ("x", "p1")))]


def test_stored_is_the_familys_store_path(monkeypatch):
    calls = []
    monkeypatch.setattr(harness, "store_yuv420_frame", lambda x, h, w: calls.append(("yuv420", x, h, w)) or ("y", "u", "v"))
    monkeypatch.setattr(harness, "store_frame", lambda x, h, w, fmt: calls.append((fmt.name, x, h, w)) or ("y", "uv"))
    assert harness.make_source("yuv420", "nowhere", 96, 64).stored("pic") == ["y", "u", "v"]
    assert harness.make_source("nv12", "nowhere", 96, 64).stored("pic") == ["y", "uv"]
    assert calls == [("yuv420", "pic", 64, 96), ("nv12", "pic", 64, 96)]
    import torch
    rgb = torch.tensor([[[0.4, 254.5, 255.0]]]).expand(3, 1, 3)
    monkeypatch.setattr(harness, "reconstruct_rgb", lambda x, h, w: calls.append(("png", x, h, w)) or rgb)
    (plane,) = harness.make_source("png", "nowhere", 96, 64).stored("pic")
    assert calls[-1] == ("png", "pic", 64, 96) and plane.dtype == torch.uint8 and plane[0, 0].tolist() == [0, 254, 255]
