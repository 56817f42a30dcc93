"""Active-area coding as far as a GPU-less host can see it (docs/active_area.md): the numpy restatement's own properties, the
host policy ActiveArea.from_extents, the NAL_ACTIVE unit written and read, the harness's option plumbing, and every C entry's
argument errors - refused by name before anything is launched."""
import ctypes
import inspect
import io
import struct

import numpy as np
import pytest

import bars_ref as R
from opendcvc_amd import _lib, bars, harness
from opendcvc_amd import bitstream as B
from opendcvc_amd.bars import ActiveArea
from opendcvc_amd.pipeline import FramePacket


# ---------------------------------------------------------------------------------- the restatement
def test_key_is_monotonic_and_puts_minus_zero_below_plus_zero():
    inf = np.float32(np.inf)
    vals = np.array([-inf, -3.0e38, -1.5, -1e-40, -0.0, 0.0, 1e-45, 1e-40, 6.1e-5, 0.5, 1.0, 6e4, 3.0e38, inf], np.float32)
    k = R.key(vals)
    assert np.all(k[1:] > k[:-1])
    assert R.key(np.float32(-0.0)) == 0x7FFFFFFF and R.key(np.float32(0.0)) == 0x80000000
    assert np.array_equal(R.value(k).view(np.uint32), vals.view(np.uint32))          # the key is a bijection of the bits
    rng = np.random.default_rng(5)
    a = rng.standard_normal(4096).astype(np.float32) * np.float32(10.0) ** rng.integers(-30, 30, 4096).astype(np.float32)
    order = np.argsort(a, kind="stable")
    assert np.all(np.diff(R.key(a)[order].astype(np.int64)) >= 0)
    h = rng.standard_normal(512).astype(np.float16)                                   # fp16 samples: the key of their fp32 value
    assert np.array_equal(R.key(h), R.key(h.astype(np.float32)))


def test_a_nan_is_an_extreme_key_and_never_a_bar():
    pos = np.array([0x7FC00000], np.uint32).view(np.float32)
    neg = np.array([0xFFC00000], np.uint32).view(np.float32)
    assert R.key(pos)[0] > R.key(np.float32(np.inf)) and R.key(neg)[0] < R.key(np.float32(-np.inf))
    assert np.isnan(R.value(R.key(pos))[0]) and np.isnan(R.value(R.key(neg))[0])
    for nan in (pos[0], neg[0]):
        x = np.full((3, 16, 24), 0.25, np.float32)
        x[:, 4:12] = np.linspace(0.3, 0.9, 24, dtype=np.float32)
        assert list(R.extent(R.scan(R.empty(16, 24), x, 16, 24), 0.0)[:5]) == [1, 4, 4, 0, 0]
        y = x.copy()
        y[1, 2, 7] = nan                                     # a NaN in a bar row: the row is no bar, whatever the tolerance
        for tol in (0.0, 1.0, np.inf):
            assert list(R.extent(R.scan(R.empty(16, 24), y, 16, 24), tol)[:5])[:2] == [1, 2]
        y = x.copy()
        y[0, 0, :] = nan                                     # row 0 all NaN: not flat, the next candidate is taken
        out = R.extent(R.scan(R.empty(16, 24), y, 16, 24), 0.0)
        assert list(out[:5]) == [1, 0, 4, 0, 0] and out[5:8].view(np.float32).tolist() == [0.25] * 3


def test_the_rule_on_hand_made_envelopes():
    x = np.full((3, 12, 20), 0.0625, np.float32)
    x[1:] = 0.5
    assert list(R.extent(R.scan(R.empty(12, 20), x, 12, 20), 0.0)[:5]) == [1, 12, 12, 20, 20]        # all bar
    x[:, 2:9, 4:18] = np.random.default_rng(0).random((3, 7, 14), np.float32) * 0.4 + 0.55
    out = R.extent(R.scan(R.empty(12, 20), x, 12, 20), 0.0)
    assert list(out[:5]) == [1, 2, 3, 4, 2] and out[5:8].view(np.float32).tolist() == [0.0625, 0.5, 0.5]
    x[:, 0, :] += np.linspace(0, 0.2, 20, dtype=np.float32)           # no flat edge line is left: found = 0, all words 0
    x[:, :, 0] += np.linspace(0.1, 0.3, 12, dtype=np.float32)
    x[:, :, 19] += np.linspace(0.1, 0.3, 12, dtype=np.float32)
    assert list(R.extent(R.scan(R.empty(12, 20), x, 12, 20), 0.0)) == [0] * 8
    assert np.array_equal(R.flat_words(R.empty(2, 3)), np.array([0xFFFFFFFF] * 15 + [0] * 15, np.uint32))


def test_window_and_paste_restatements_invert_each_other():
    rng = np.random.default_rng(1)
    x = np.full((3, 32, 48), 0.5, np.float16)
    x[0] = 0.0625
    x[:, 4:26, 6:40] = rng.random((3, 22, 34)).astype(np.float16)
    w = R.window(x, 4, 6, 22, 34, 32, 48)
    assert np.array_equal(w[:, :22, :34], x[:, 4:26, 6:40]) and np.array_equal(w[:, 31, 47], x[:, 25, 39])
    back = R.paste(w, 22, 34, 4, 6, 32, 48, 32, 48, (0.0625, 0.5, 0.5))
    assert np.array_equal(back, x)


# ---------------------------------------------------------------------------------- the host policy
COL = (0.0625, 0.5, 0.5)


def test_from_extents_rounds_down_to_even():
    a = ActiveArea.from_extents(1080, 1920, (139, 137, 3, 0, COL))
    assert (a.full_height, a.full_width, a.top, a.left, a.height, a.width, a.colour) == (1080, 1920, 138, 2, 806, 1918, COL)
    assert a.extents == [138, 136, 2, 0] and a.size == (806, 1918) and a.full_size == (1080, 1920)
    with pytest.raises(Exception):
        a.top = 0                                            # frozen


def test_from_extents_keeps_a_dimension_that_would_fall_below_min_size():
    a = ActiveArea.from_extents(128, 256, (40, 40, 20, 20, COL))                # 48 rows would be left: rows are kept
    assert (a.top, a.height, a.left, a.width) == (0, 128, 20, 216)
    a = ActiveArea.from_extents(128, 256, (40, 40, 20, 20, COL), min_size=48)
    assert (a.top, a.height, a.left, a.width) == (40, 48, 20, 216)
    a = ActiveArea.from_extents(256, 128, (40, 40, 40, 40, COL))                # ... and columns, each on its own
    assert (a.top, a.height, a.left, a.width) == (40, 176, 0, 128)
    assert ActiveArea.from_extents(128, 128, (40, 40, 40, 40, COL)) is None


def test_from_extents_of_nothing_to_crop_is_none():
    assert ActiveArea.from_extents(128, 160, None) is None
    assert ActiveArea.from_extents(128, 160, (0, 0, 0, 0, COL)) is None
    assert ActiveArea.from_extents(128, 160, (1, 1, 1, 0, COL)) is None          # below one chroma sample
    assert ActiveArea.from_extents(128, 160, (128, 128, 160, 160, COL)) is None  # all bar
    assert ActiveArea.from_extents(128, 160, (128, 128, 160, 160, COL), min_size=0) is None


def test_an_active_area_refuses_a_window_outside_or_at_odd_offsets():
    for bad in ((64, 64, 2, 0, 64, 64), (64, 64, 0, 0, 0, 64), (64, 64, 1, 0, 32, 64), (64, 64, 0, 3, 64, 32), (64, 64, 0, 2, 64, 64)):
        with pytest.raises(ValueError):
            ActiveArea(*bad, COL)


# ---------------------------------------------------------------------------------- the unit
AREA = ActiveArea(1080, 1920, 138, 0, 804, 1920, (16 / 255, 0.5, -2.5))
UNIT = bytes([0x83, 0x84, 0x38, 0x87, 0x80, 0x80, 0x8A, 0x00]) + struct.pack("<3f", np.float32(16 / 255), 0.5, -2.5)


def _pkt(is_i=True, payload=b"\x01\x02"):
    return FramePacket(is_i, 30, 0, payload)


def test_unit_bytes_known_answer_and_read_back():
    f = io.BytesIO()
    assert B.write_active(f, 3, AREA) == len(UNIT) == 20 and f.getvalue() == UNIT
    assert int(B.NalType.NAL_ACTIVE) == 8
    area = ActiveArea(1080, 1920, 138, 0, 804, 1920, struct.unpack("<3f", UNIT[8:]))
    f = io.BytesIO()
    w = B.StreamWriter(f, active=area)
    n = w.write_frame(804, 1920, True, _pkt()) + w.write_frame(804, 1920, True, _pkt(False, b"\x03"))
    data = f.getvalue()
    assert n == len(data)
    sps = io.BytesIO()
    B.write_sps(sps, dict(sps_id=0, height=804, width=1920, use_ada_i=0, ec_part=1))
    assert data.startswith(sps.getvalue() + bytes([0x80]) + UNIT[1:]) and data.count(UNIT[1:]) == 1      # behind the SPS, once
    rd = B.StreamReader(io.BytesIO(data))
    assert rd.active is None
    for _ in range(2):
        got_sps, pkt = rd.read_packet()
        assert (got_sps["height"], got_sps["width"]) == (804, 1920) and rd.active == area and rd.display is None
    assert B.frame_overhead_bytes(2) == 3


def test_the_unit_follows_the_display_unit_and_takes_its_size():
    area = ActiveArea(128, 160, 32, 0, 64, 160, COL)
    f = io.BytesIO()
    w = B.StreamWriter(f, display=(64, 160, "bicubic"), active=area)
    w.write_frame(32, 80, False, _pkt())
    w.write_frame(32, 80, False, _pkt(False))
    w.write_frame(48, 80, False, _pkt())                      # a second SPS: display and active-area units again
    data = f.getvalue()
    assert [data[i] >> 4 for i in (0, 4, 9)] == [0, 6, 8]
    rd = B.StreamReader(io.BytesIO(data))
    for want_sps in (0, 0, 1):
        sps, _ = rd.read_packet()
        assert sps["sps_id"] == want_sps and rd.display == (64, 160, "bicubic") and rd.active == area
    with pytest.raises(ValueError, match="window"):
        B.StreamWriter(io.BytesIO(), active=area).write_frame(32, 80, False, _pkt())      # not the pictures' size


def test_active_follows_the_frames_sps_as_display_does():
    area = ActiveArea(64, 64, 16, 0, 32, 64, COL)
    f = io.BytesIO()
    B.write_sps(f, dict(sps_id=0, height=32, width=64, use_ada_i=0, ec_part=0))
    B.write_active(f, 0, area)
    B.write_ip(f, True, 0, 30, b"a")
    B.write_sps(f, dict(sps_id=1, height=64, width=64, use_ada_i=0, ec_part=0))          # no unit behind this one
    B.write_ip(f, True, 1, 30, b"b")
    B.write_ip(f, False, 0, 30, b"c")
    B.write_sps(f, dict(sps_id=0, height=32, width=64, use_ada_i=1, ec_part=0))          # id 0 anew: its unit is gone
    B.write_ip(f, False, 0, 30, b"d")
    rd = B.StreamReader(io.BytesIO(f.getvalue()))
    seen = []
    for _ in range(4):
        rd.read_frame()
        seen.append(rd.active)
    assert seen == [area, None, area, None]


def _stream(unit, sps_id=0, height=804, width=1920, display=None):
    f = io.BytesIO()
    B.write_sps(f, dict(sps_id=sps_id, height=height, width=width, use_ada_i=0, ec_part=1))
    if display:
        B.write_display(f, sps_id, *display)
    f.write(unit)
    B.write_ip(f, True, sps_id, 30, b"\x00" * 40)
    return io.BytesIO(f.getvalue())


def _unit(sps_id, full_h, full_w, top, left, colour=COL):
    f = io.BytesIO()
    f.write(bytes([0x80 | sps_id]))
    for v in (full_h, full_w, top, left):
        B.write_uint_adaptive(f, v)
    f.write(struct.pack("<3f", *colour))
    return f.getvalue()


def test_reader_errors():
    B.StreamReader(_stream(_unit(0, 1080, 1920, 138, 0))).read_frame()                  # the good one
    with pytest.raises(ValueError, match="unknown SPS"):
        B.StreamReader(_stream(_unit(5, 1080, 1920, 138, 0))).read_frame()
    for full_h, full_w, top, left in ((940, 1920, 138, 0), (1080, 1900, 138, 0), (1080, 1920, 278, 0), (1080, 1930, 0, 12)):
        with pytest.raises(ValueError, match="not inside"):
            B.StreamReader(_stream(_unit(0, full_h, full_w, top, left))).read_frame()
    for top, left in ((137, 0), (138, 1)):
        with pytest.raises(ValueError, match="even"):
            B.StreamReader(_stream(_unit(0, 1080, 1924, top, left))).read_frame()
    good = _unit(0, 1080, 1920, 138, 0)
    for cut in range(1, len(good)):
        f = io.BytesIO()
        B.write_sps(f, dict(sps_id=0, height=804, width=1920, use_ada_i=0, ec_part=1))
        f.write(good[:cut])
        with pytest.raises(ValueError, match="truncated"):
            B.StreamReader(io.BytesIO(f.getvalue())).read_frame()
    # the order is normative: a display unit behind the active-area unit of its SPS would change the window's size after the check
    f = io.BytesIO()
    B.write_sps(f, dict(sps_id=0, height=402, width=960, use_ada_i=0, ec_part=1))
    f.write(_unit(0, 540, 960, 68, 0))                                  # valid at the SPS's own size
    B.write_display(f, 0, 804, 1920, "lanczos3")
    B.write_ip(f, True, 0, 30, b"\x00")
    with pytest.raises(ValueError, match="display unit follows"):
        B.StreamReader(io.BytesIO(f.getvalue())).read_frame()
    # the window is the display unit's size where the SPS has one
    B.StreamReader(_stream(good, height=402, width=960, display=(804, 1920, "lanczos3"))).read_frame()
    with pytest.raises(ValueError, match="not inside"):
        B.StreamReader(_stream(_unit(0, 600, 1920, 138, 0), height=402, width=960, display=(804, 1920, "lanczos3"))).read_frame()


def test_a_stream_without_the_unit_is_written_and_parsed_as_before():
    def write(**kw):
        f = io.BytesIO()
        w = B.StreamWriter(f, **kw)
        for i, pkt in enumerate((_pkt(), _pkt(False, b"\x05" * 300))):
            w.write_frame(64, 80, False, pkt)
        return f.getvalue()
    assert write() == write(active=None) == write(display=None, active=None)
    rd = B.StreamReader(io.BytesIO(write()))
    assert [rd.read_frame()[3] for _ in range(2)] == [b"\x01\x02", b"\x05" * 300] and rd.active is None and rd.display is None
    assert "active" in inspect.signature(B.StreamWriter.__init__).parameters


# ---------------------------------------------------------------------------------- the harness's options
def test_crop_kwargs_and_the_parser_spellings():
    assert harness.crop_kwargs({}) == {} and harness.crop_kwargs(dict(crop=None, crop_tol=None)) == {}
    assert harness.crop_kwargs(dict(crop=None, crop_tol=2.0)) == {}
    assert harness.crop_kwargs(dict(crop="auto", crop_tol=None, other=1)) == {"crop": "auto"}
    assert harness.crop_kwargs(dict(crop="auto", crop_tol=1.5)) == {"crop": "auto", "crop_tol": 1.5}
    ap = harness.build_parser()
    base = "--src a.yuv --width 64 --height 64 --frames 1".split()
    assert harness.crop_kwargs(vars(ap.parse_args(base))) == {}
    assert harness.crop_kwargs(vars(ap.parse_args(base + ["--crop", "auto"]))) == {"crop": "auto"}
    assert harness.crop_kwargs(vars(ap.parse_args(base + "--crop 138:138:0:0 --crop-tol 2".split()))) == \
        {"crop": (138, 138, 0, 0, (16, 128, 128)), "crop_tol": 2.0}
    assert harness.crop_kwargs(vars(ap.parse_args(base + "--crop 0:0:8:10:0:128:128 --crop_tol 0".split()))) == \
        {"crop": (0, 0, 8, 10, (0, 128, 128))}
    for bad in ("137:138:0:0", "1:2:3", "a:b:c:d", "2:2:2:2:16:128", "2:2:2:2:16:128:256", "Auto", "-2:0:0:0"):
        with pytest.raises(ValueError):
            harness.parse_crop(bad)
        with pytest.raises(SystemExit):
            ap.parse_args(base + ["--crop", bad])
    args = ap.parse_args("--test-config m.json --gpus 1 --gpu-ids 0 --crop auto".split())
    opts, _ = harness.manifest_options(args, ap)
    assert opts["crop"] == "auto" and "crop_tol" not in opts
    opts, _ = harness.manifest_options(ap.parse_args("--test-config m.json --gpus 1 --gpu-ids 0".split()), ap)
    assert "crop" not in opts and "crop_tol" not in opts
    params = inspect.signature(harness.run_one_point).parameters
    assert params["crop"].default is None and params["crop_tol"].default == 0.0
    assert [n for n, _, _ in harness.POINT_OPTIONS][-1] == "film_grain"               # the table is not where it travels


def test_check_crop():
    assert harness.check_crop(None, 0.0, 128, 160) == (None, 0.0)
    assert harness.check_crop("auto", 2.0, 128, 160) == ("auto", float(np.float32(2.0) / np.float32(255.0)))
    area, tol = harness.check_crop((32, 32, 0, 0, (16, 128, 128)), 0.0, 128, 160)
    assert area == ActiveArea(128, 160, 32, 0, 64, 160, tuple(float(np.float32(c) / np.float32(255.0)) for c in (16, 128, 128)))
    assert harness.check_crop("32:32:0:0", 0.0, 128, 160)[0] == area
    assert harness.check_crop((0, 0, 0, 0, (16, 128, 128)), 0.0, 128, 160)[0] is None
    for bad in ((64, 64, 0, 0, (16, 128, 128)), (1, 1, 0, 0, (16, 128, 128)), (2, 2, 0, 0), "nonsense"):
        with pytest.raises(ValueError):
            harness.check_crop(bad, 0.0, 128, 160)
    with pytest.raises(ValueError):
        harness.check_crop("auto", -1.0, 128, 160)
    for crop in (None, "32:32:0:0", (32, 32, 0, 0, (16, 128, 128))):          # the tolerance belongs to the detection
        with pytest.raises(ValueError, match="no effect"):
            harness.check_crop(crop, 1.0, 128, 160)


def test_crop_tol_without_crop_auto_is_a_usage_error(monkeypatch):
    monkeypatch.setattr(harness, "run_sweep", lambda *a, **kw: {})
    import os
    base = f"--src a.yuv --width 64 --height 64 --frames 1 --out {os.devnull}".split()
    harness.main(base + "--crop auto --crop-tol 1.5".split())
    for extra in ("--crop-tol 1.5", "--crop 2:2:0:0 --crop-tol 1.5", "--crop auto --crop-tol -1"):
        with pytest.raises(SystemExit):
            harness.main(base + extra.split())


def test_without_crop_run_one_point_gets_no_new_keyword(monkeypatch):
    seen = []
    monkeypatch.setattr(harness, "run_one_point", lambda *a, **kw: seen.append(kw) or {})
    monkeypatch.setattr(harness, "run_sweep", lambda *a, **kw: seen.append(kw) or {})
    job = dict(src_path="x.yuv", src_width=64, src_height=64, frame_num=2, qp_i=32, qp_p=32, intra_period=-1, reset_interval=32)
    import os
    harness.run_job(("i", "p"), job, {})
    harness.main(f"--src a.yuv --width 64 --height 64 --frames 1 --out {os.devnull}".split())
    harness.run_job(("i", "p"), job, {"crop": "auto", "crop_tol": 1.0})
    harness.main(f"--src a.yuv --width 64 --height 64 --frames 1 --crop 2:2:0:0 --out {os.devnull}".split())
    for kw in seen[:2]:
        assert "crop" not in kw and "crop_tol" not in kw
    assert (seen[2]["crop"], seen[2]["crop_tol"]) == ("auto", 1.0)
    assert seen[3]["crop"] == (2, 2, 0, 0, (16, 128, 128)) and "crop_tol" not in seen[3]


# ---------------------------------------------------------------------------------- the C entries' argument errors
# a 64-byte-aligned host buffer stands in for every pointer: each call below must be refused before anything is launched
_BUF = ctypes.create_string_buffer(65536 + 64)
_PTR = (ctypes.addressof(_BUF) + 63) & ~63
_A, _B, _C = _PTR, _PTR + 24576, _PTR + 49152             # a frame of 3 * 32 * 48 fp16 elements is 9216 bytes
_COLOUR = (ctypes.c_float * 3)(0.0625, 0.5, 0.5)


def _ws_bytes(H=30, W=40):
    return _lib.lib().dcvc_bars_ws_bytes(H, W)


def _reset(ws=_C, H=30, W=40):
    return _lib.lib().dcvc_bars_reset(ws, H, W, None)


def _scan(dtype=_lib.F16, x=_A, Hp=32, Wp=48, H=30, W=40, ws=_C):
    return _lib.lib().dcvc_bars_scan(dtype, x, Hp, Wp, H, W, ws, None)


def _extent(ws=_C, H=30, W=40, tol=0.0, out=_B):
    return _lib.lib().dcvc_bars_extent(ws, H, W, tol, out, None)


def _window(dtype=_lib.F16, x=_A, Hp=32, Wp=48, H=30, W=40, top=2, left=4, out=_B, HOp=32, WOp=32, HO=20, WO=30):
    return _lib.lib().dcvc_frame_window(dtype, x, Hp, Wp, H, W, top, left, out, HOp, WOp, HO, WO, None)


def _paste(dtype=_lib.F16, x=_A, Hp=32, Wp=32, H=20, W=30, out=_B, HOp=32, WOp=48, HO=30, WO=40, top=2, left=4, colour=_COLOUR):
    return _lib.lib().dcvc_frame_paste(dtype, x, Hp, Wp, H, W, out, HOp, WOp, HO, WO, top, left, colour, None)


FRAME_ERRORS = [dict(dtype=_lib.U8), dict(x=None), dict(x=_A + 1), dict(H=0), dict(W=-1), dict(Hp=8), dict(Wp=8)]
BAD = {
    "dcvc_bars_ws_bytes": (_ws_bytes, [dict(H=0), dict(W=0), dict(H=(1 << 20) + 1), dict(W=-5)]),
    "dcvc_bars_reset": (_reset, [dict(ws=None), dict(ws=_C + 2), dict(H=0), dict(W=(1 << 20) + 1)]),
    "dcvc_bars_scan": (_scan, FRAME_ERRORS + [dict(ws=None), dict(ws=_C + 1), dict(Hp=1 << 20, Wp=1 << 20)]),
    "dcvc_bars_extent": (_extent, [dict(ws=None), dict(ws=_C + 2), dict(H=0), dict(W=0), dict(tol=-1.0), dict(tol=float("nan")),
                                   dict(out=None), dict(out=_B + 2)]),
    "dcvc_frame_window": (_window, FRAME_ERRORS + [dict(out=None), dict(out=_B + 8), dict(WOp=36), dict(HO=0), dict(WO=0),
                                                   dict(HOp=16), dict(WOp=24), dict(top=-2), dict(left=-2), dict(top=12),
                                                   dict(left=12), dict(HO=29, HOp=32), dict(WO=38, WOp=40)]),
    "dcvc_frame_paste": (_paste, FRAME_ERRORS + [dict(out=None), dict(out=_B + 8), dict(WOp=44), dict(HO=0), dict(HOp=16),
                                                 dict(WOp=32), dict(colour=None), dict(top=-2), dict(left=-2), dict(top=12),
                                                 dict(left=12), dict(out=_A), dict(out=_A + 6144 - 16), dict(x=_B + 9216 - 16)]),
}
CASES = [pytest.param(name, call, kw, id=f"{name}-{'-'.join(f'{k}' for k in kw)}-{i}")
         for name, (call, kws) in BAD.items() for i, kw in enumerate(kws)]


@pytest.mark.parametrize("name, call, kw", CASES)
def test_a_bad_argument_is_refused_by_name_before_any_launch(name, call, kw):
    before = bytes(_BUF)
    assert call(**kw) == -1, (name, kw)
    err = _lib.lib().dcvc_last_error()
    assert name.encode() in err, err
    assert bytes(_BUF) == before


def test_ws_bytes():
    assert _ws_bytes() == 24 * 70 and _ws_bytes(1080, 1920) == 24 * 3000 and _ws_bytes(1, 1) == 48
    for name in ("dcvc_bars_ws_bytes", "dcvc_bars_reset", "dcvc_bars_scan", "dcvc_bars_extent", "dcvc_frame_window",
                 "dcvc_frame_paste"):
        assert name in _lib.EXPORTS
    assert bars.BarDetector and bars.window and bars.paste
