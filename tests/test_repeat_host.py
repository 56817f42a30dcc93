"""Repeated-frame coding as far as a GPU-less host can see it (docs/frame_repeat.md): the numpy restatement's own properties,
the NAL_REPEAT unit written and read, RateController.skip, SequenceEncoder.repeat() / SequenceDecoder.decode() on stub codecs,
the harness's option plumbing, and dcvc_frame_maxdiff's argument errors - refused by name before anything is launched."""
import ctypes
import inspect
import io
import os

import numpy as np
import pytest

import repeat_ref as R
from opendcvc_amd import _lib, harness, pipeline, repeat
from opendcvc_amd import bitstream as B
from opendcvc_amd.grain import GrainParams
from opendcvc_amd.pipeline import FramePacket, SequenceDecoder, SequenceEncoder
from opendcvc_amd.ratecontrol import I_CLASS, RateController


# ---------------------------------------------------------------------------------- the restatement
def test_the_restatement_on_hand_made_frames():
    a = np.full((3, 8, 16), 0.5, np.float32)
    b = a.copy()
    assert R.maxdiff(a, b, 6, 10).tolist() == [0, 0, 0, 0]
    b[1, 2, 3] = 0.75
    b[2, 7, 15] = 9.0                                     # the padding does not count
    b[0, 5, 9] = -0.0
    a[0, 5, 9] = 0.0                                      # +0 against -0: key 0
    a[0, 0, 0], b[0, 0, 0] = 0.0, -0.0
    assert R.maxdiff(a, b, 6, 10).tolist() == [0, int(np.float32(0.25).view(np.uint32)), 0, 0]
    b[0, 1, 1] = np.nan
    a[2, 1, 1] = b[2, 1, 1] = np.inf                      # inf - inf is a NaN
    keys = R.maxdiff(a, b, 6, 10)
    assert keys[0] > 0x7F800000 and keys[2] > 0x7F800000 and keys[3] == 0
    for tol in (0.0, 255.0, np.inf):
        assert not R.is_repeat(keys, tol)                 # a NaN passes no tolerance
    h = np.random.default_rng(0).random((3, 8, 16)).astype(np.float16)
    g = h.copy()
    g[1, 0, 0] = np.float16(float(h[1, 0, 0]) + 0.25)
    want = np.abs(np.float32(g[1, 0, 0]) - np.float32(h[1, 0, 0])).view(np.uint32)
    assert R.maxdiff(h, g, 8, 16).tolist() == [0, int(want), 0, 0]          # fp16 samples: the difference of their fp32 values
    assert R.is_repeat(R.maxdiff(h, g, 8, 16), 64.0) and not R.is_repeat(R.maxdiff(h, g, 8, 16), 63.0)


def test_tol_fraction_is_check_crops_conversion():
    for tol in (0.0, 1.0, 1.5, 3.0):
        assert repeat.tol_fraction(tol) == float(np.float32(tol) / np.float32(255)) == harness.check_crop("auto", tol, 64, 64)[1]
    for bad in (-1.0, float("nan"), -1e-9):
        with pytest.raises(ValueError):
            repeat.tol_fraction(bad)


# ---------------------------------------------------------------------------------- the unit
P1 = GrainParams(7, 1, (10, 20, 30, 40, 50, 60, 70, 80), 9, 11)


def _pkt(is_i=True, payload=b"\x01\x02", **kw):
    return FramePacket(is_i, 30, 0, payload, **kw)


REP = FramePacket(False, 0, 0, b"", repeat=True)


def test_unit_known_answer_written_and_read():
    assert int(B.NalType.NAL_REPEAT) == 9 and B.REPEAT_UNIT_BYTES == 1
    f = io.BytesIO()
    assert B.write_repeat(f, 3) == 1 and f.getvalue() == bytes([0x93])
    for bad in (-1, 16):
        with pytest.raises(ValueError):
            B.write_repeat(io.BytesIO(), bad)
    assert FramePacket(True, 1, 0, b"x").repeat is False and REP.repeat

    f = io.BytesIO()
    w = B.StreamWriter(f, display=(64, 96, "bicubic"))
    sizes = [w.write_frame(32, 48, False, _pkt(grain=P1, digest=5)), w.write_frame(32, 48, False, REP),
             w.write_frame(32, 48, False, REP), w.write_frame(32, 48, False, _pkt(False, b"\x07" * 5)),
             w.write_frame(16, 16, False, _pkt()), w.write_frame(16, 16, False, REP)]
    data = f.getvalue()
    assert sizes[1] == sizes[2] == sizes[5] == 1 and sum(sizes) == len(data)
    at = sizes[0]
    assert data[at:at + 2] == bytes([0x90, 0x90]) and data[-1] == 0x91       # the header byte alone, the SPS of the frame before
    rd = B.StreamReader(io.BytesIO(data))
    assert rd.repeat is False
    seen = []
    for _ in range(6):
        sps, is_i, qp, payload = rd.read_frame()
        seen.append((sps["sps_id"], sps["height"], is_i, qp, payload, rd.repeat, rd.chunked, rd.digest, rd.grain_t, rd.display))
    big, small = (64, 96, "bicubic"), (64, 96, "bicubic")
    assert seen == [(0, 32, True, 30, b"\x01\x02", False, False, 5, 0, big),
                    (0, 32, False, 0, b"", True, False, None, 1, big),
                    (0, 32, False, 0, b"", True, False, None, 2, big),      # grain_t goes on: the grain does not freeze
                    (0, 32, False, 30, b"\x07" * 5, False, False, None, 3, big),
                    (1, 16, True, 30, b"\x01\x02", False, False, None, 4, small),
                    (1, 16, False, 0, b"", True, False, None, 5, small)]
    assert rd.grain == P1
    with pytest.raises(EOFError):
        rd.read_frame()
    rd = B.StreamReader(io.BytesIO(data))
    pkts = [rd.read_packet()[1] for _ in range(6)]
    assert [p.repeat for p in pkts] == [False, True, True, False, False, True] and pkts[1] == REP


def test_active_area_of_a_repeat_is_its_sps():
    from opendcvc_amd.bars import ActiveArea
    area = ActiveArea(64, 48, 16, 0, 32, 48, (0.0625, 0.5, 0.5))
    f = io.BytesIO()
    w = B.StreamWriter(f, active=area)
    w.write_frame(32, 48, False, _pkt())
    w.write_frame(32, 48, False, REP)
    rd = B.StreamReader(io.BytesIO(f.getvalue()))
    rd.read_frame()
    assert rd.active == area and not rd.repeat
    rd.read_frame()
    assert rd.active == area and rd.repeat and rd.display is None


def test_writer_errors():
    w = B.StreamWriter(io.BytesIO())
    with pytest.raises(ValueError, match="in front of any frame"):
        w.write_frame(32, 48, False, REP)
    w.write_frame(32, 48, False, _pkt())
    with pytest.raises(ValueError, match="behind a frame of"):
        w.write_frame(16, 48, False, REP)
    n = len(w.f.getvalue())
    # no SPS, digest or grain unit is ever written for a repeat, whatever the packet carries
    assert w.write_frame(32, 48, False, FramePacket(False, 0, 1, b"", repeat=True, grain=P1, digest=9)) == 1
    assert w.f.getvalue()[n:] == bytes([0x90])


def _frame_then(units):
    f = io.BytesIO()
    B.write_sps(f, dict(sps_id=0, height=32, width=48, use_ada_i=0, ec_part=0))
    B.write_ip(f, True, 0, 30, b"ab")
    for u in units:
        u(f)
    return B.StreamReader(io.BytesIO(f.getvalue()))


def test_reader_errors():
    rd = _frame_then([lambda f: B.write_repeat(f, 0)])
    rd.read_frame()
    assert rd.read_frame() == (rd.sps_helper.get_sps_by_id(0), False, 0, b"") and rd.repeat
    rd = _frame_then([lambda f: B.write_digest(f, 0, 77), lambda f: B.write_repeat(f, 0)])
    rd.read_frame()
    with pytest.raises(ValueError, match="a digest unit is followed by NAL_REPEAT"):
        rd.read_frame()
    rd = _frame_then([lambda f: B.write_grain(f, 0, P1), lambda f: B.write_repeat(f, 0)])
    rd.read_frame()
    with pytest.raises(ValueError, match="a grain unit is followed by NAL_REPEAT"):
        rd.read_frame()
    rd = _frame_then([lambda f: B.write_repeat(f, 5)])
    rd.read_frame()
    with pytest.raises(ValueError, match="unknown SPS"):
        rd.read_frame()
    with pytest.raises(ValueError, match="unknown SPS"):
        B.StreamReader(io.BytesIO(bytes([0x90]))).read_frame()
    f = io.BytesIO()
    B.write_sps(f, dict(sps_id=0, height=32, width=48, use_ada_i=0, ec_part=0))
    B.write_repeat(f, 0)
    with pytest.raises(ValueError, match="before the first frame"):
        B.StreamReader(io.BytesIO(f.getvalue())).read_frame()
    # the unit names the picture it repeats: the SPS of the frame before, no other
    rd = _frame_then([lambda f: B.write_sps(f, dict(sps_id=1, height=16, width=16, use_ada_i=0, ec_part=0)),
                      lambda f: B.write_repeat(f, 1)])
    rd.read_frame()
    with pytest.raises(ValueError, match="the frame before it has SPS 0"):
        rd.read_frame()


def test_a_stream_without_the_unit_is_written_and_parsed_as_before():
    f = io.BytesIO()
    w = B.StreamWriter(f)
    n = w.write_frame(64, 80, False, _pkt()) + w.write_frame(64, 80, False, _pkt(False, b"\x05" * 300))
    g = io.BytesIO()
    B.write_sps(g, dict(sps_id=0, height=64, width=80, use_ada_i=0, ec_part=0))
    B.write_ip(g, True, 0, 30, b"\x01\x02")
    B.write_ip(g, False, 0, 30, b"\x05" * 300)
    assert f.getvalue() == g.getvalue() and n == len(g.getvalue())
    rd = B.StreamReader(io.BytesIO(f.getvalue()))
    assert [rd.read_frame()[3] for _ in range(2)] == [b"\x01\x02", b"\x05" * 300] and rd.repeat is False


# ---------------------------------------------------------------------------------- RateController.skip
def test_skip_moves_the_debt_and_leaves_the_model():
    rc = RateController(1000.0, 30)
    rc.observe(I_CLASS, 30, 5000)
    rc.observe(0, 30, 900)
    before = dict(vars(rc), _class=dict(rc._class), _last=dict(rc._last), exact_bytes=list(rc.exact_bytes))
    rc.skip(8)
    after = dict(vars(rc))
    assert after["debt"] == before["debt"] + 8 - 1000.0 and after["frames"] == before["frames"] + 1
    for k in before:
        if k not in ("debt", "frames"):
            assert after[k] == before[k], k


def test_a_skip_of_target_bits_leaves_the_trace_of_later_frames():
    def trace(interposed):
        rc = RateController(1000.0, 30, qp_i_init=26)
        out = []
        sizes = [(I_CLASS, 6000), (0, 1400), (1, 1300), (0, 900), (2, 1100), (0, 1000), (2, 700), (0, 1250), (2, 950)]
        for i, (klass, bits) in enumerate(sizes):
            base = rc.base_qp()
            out.append(base)
            rc.observe(klass, base, bits * (1.0 + 0.02 * (30 - base)))
            if interposed and i in (2, 3, 6):
                rc.skip(rc.target)                        # a frame exactly on budget: the debt stays
        out.append(rc.base_qp())
        return out, rc
    plain, a = trace(False)
    skipped, b = trace(True)
    assert plain == skipped and len(set(plain)) > 2       # (the trace does move)
    assert (a.b, a._level, a._anchor, a._class, a.debt) == (b.b, b._level, b._anchor, b._class, b.debt)
    assert b.frames == a.frames + 3


# ---------------------------------------------------------------------------------- SequenceEncoder.repeat / SequenceDecoder.decode
class _Stubs:
    """stub codecs: every call recorded; a P compress with defer_stream holds its stream back as DMC does"""

    def __init__(self):
        self.calls = []
        outer = self

        class I:
            def compress(self, x, qp):
                outer.calls.append(("i", x, qp))
                return dict(bit_stream=b"I%d" % x, x_hat="rec", est_bytes=500)

            def decompress(self, bit_stream, sps, qp):
                outer.calls.append(("di", bit_stream))
                return dict(x_hat="pic-" + bit_stream.decode())

        class P:
            pending = None           # encoder side: the stream held back
            pending_out = None       # decoder side: the picture held back

            def set_curr_poc(self, poc):
                pass

            def clear_dpb(self):
                outer.calls.append("clear_dpb")

            def add_ref_frame(self, feature, frame):
                outer.calls.append("add_ref_frame")

            def prepare_feature_adaptor_i(self, last_qp):
                outer.calls.append("adaptor_i")

            def reset_ref_feature(self):
                pass

            def shift_qp(self, qp, fa_idx):
                return qp + fa_idx

            def finish_stream(self):
                s, self.pending = self.pending, None
                return s

            def finish_output(self):
                s, self.pending_out = self.pending_out, None
                return s

            def compress(self, x, qp, defer_stream=False):
                outer.calls.append(("p", x, qp))
                stream = b"P%d" % x
                if not defer_stream:
                    return dict(bit_stream=stream, est_bytes=100)
                prev, self.pending = self.pending, stream
                return dict(bit_stream=None, bit_stream_prev=prev, est_bytes=100)

            def decompress(self, bit_stream, sps, qp, defer_output=False):
                outer.calls.append(("dp", bit_stream))
                pic = "pic-" + bit_stream.decode()
                if not defer_output:
                    return dict(x_hat=pic)
                prev, self.pending_out = self.pending_out, pic
                return dict(x_hat_prev=prev, x_hat=None)

        self.i, self.p = I(), P()


KW = dict(intra_period=4, reset_interval=3)
# source frames 0 .. 9, "r" a repeat of the frame before it
CLIP = [0, "r", 1, 2, "r", "r", 3, 4, "r", 5, 6, 7, "r", 8, 9]


def _counters(enc):
    return enc.frame_idx, enc._gop_pos, enc.last_qp, list(enc.scene_cuts)


@pytest.mark.parametrize("scenecut", [0, 150])
def test_repeat_moves_no_counter_and_the_coded_frames_are_those_of_the_clip_without_it(scenecut):
    kw = dict(KW, scenecut=scenecut, min_keyint=2) if scenecut else KW
    cut = (lambda x: dict(cut=x in (6,))) if scenecut else (lambda x: {})
    st, plain = _Stubs(), _Stubs()
    enc, ref = SequenceEncoder(st.i, st.p, 20, 30, **kw), SequenceEncoder(plain.i, plain.p, 20, 30, **kw)
    with pytest.raises(ValueError, match="before the first frame"):
        enc.repeat()
    got, want = [], [ref.encode(x, **cut(x)) for x in CLIP if x != "r"]
    for x in CLIP:
        if x == "r":
            before, calls = _counters(enc), list(st.calls)
            pkt = enc.repeat()
            assert pkt == FramePacket(False, 0, 0, b"", repeat=True)
            assert _counters(enc) == before and st.calls == calls            # nothing moved, nothing was called
        else:
            pkt = enc.encode(x, **cut(x))
        got.append(pkt)
    assert [p for p in got if not p.repeat] == want and st.calls == plain.calls
    assert [p.repeat for p in got] == [x == "r" for x in CLIP]
    assert sum(p.is_i for p in want) >= 3 and sum(p.use_ada_i for p in want) >= 2       # (the rules were exercised)


def test_repeat_with_defer_stream_finishes_the_held_packet_first():
    st, plain = _Stubs(), _Stubs()
    enc = SequenceEncoder(st.i, st.p, 20, 30, defer_stream=True, **KW)
    ref = SequenceEncoder(plain.i, plain.p, 20, 30, **KW)
    got = []
    for x in CLIP:
        out = enc.repeat() if x == "r" else enc.encode(x)
        assert isinstance(out, list)
        got += out
    got += enc.flush()
    want = []
    for x in CLIP:
        want.append(FramePacket(False, 0, 0, b"", repeat=True) if x == "r" else ref.encode(x))
    assert got == want                                                       # every packet, in source order
    # a repeat right behind a P frame hands out that frame's packet with it
    enc = SequenceEncoder(st.i, st.p, 20, 30, defer_stream=True, **KW)
    assert [p.bit_stream for p in enc.encode(0)] == [b"I0"] and enc.encode(1) == []
    out = enc.repeat()
    assert [p.bit_stream for p in out] == [b"P1", b""] and out[1].repeat and enc.repeat() == [out[1]] and enc.flush() == []


def test_repeat_under_rate_control():
    class Rate(RateController):
        def __init__(self):
            super().__init__(4000.0, 30, qp_i_init=26)
            self.log = []

        def observe(self, klass, base, bits):
            self.log.append(("observe", klass, bits))
            super().observe(klass, base, bits)

        def skip(self, bits):
            self.log.append(("skip", bits))
            super().skip(bits)

    st = _Stubs()
    rate = Rate()
    enc = SequenceEncoder(st.i, st.p, 26, 30, rate=rate)
    pkts = [enc.encode(0), enc.repeat(), enc.repeat(), enc.encode(1), enc.repeat(), enc.encode(2)]
    debt = rate.debt
    assert rate.log[:3] == [("observe", I_CLASS, 8 * 504), ("skip", 8), ("skip", 8)]       # the pending observation first
    assert rate.log[3:] == [("observe", 1, 8 * 103), ("skip", 8)] and rate.frames == 5     # INDEX_MAP[1]: coded frame 1
    assert debt == (8 * 504 - 4000.0) + 3 * (8 - 4000.0) + (8 * 103 - 4000.0)
    assert enc.rc_qp == [pkts[0].qp] * 3 + [pkts[3].qp] * 2 + [pkts[5].qp]                 # a repeat repeats the last qp
    assert enc.rc_est_bytes == [504, 1, 1, 103, 1, 103]
    assert enc.rc_bytes == [2 + 3, 1, 1, 2 + 3, 1, 2 + 3]                                  # no frame header for a repeat
    assert [i for i, _ in rate.exact_bytes] == list(range(6))


def test_decoder_returns_the_previous_picture_and_touches_nothing():
    st = _Stubs()
    dec = SequenceDecoder(st.i, st.p, 32, 48, False)
    with pytest.raises(_lib.DcvcError, match="before any picture"):
        dec.decode(FramePacket(False, 0, 0, b"", repeat=True))
    assert dec.frame_idx == 1
    a = dec.decode(FramePacket(True, 30, 0, b"I0"))
    calls = list(st.calls)
    b = dec.decode(REP)
    c = dec.decode(REP)
    assert a == "pic-I0" and b is a and c is a and st.calls == calls and dec.frame_idx == 4
    assert dec._unchecked == [] and dec.digests_checked == 0 and dec._digester is None
    d = dec.decode(FramePacket(False, 31, 0, b"P1"))
    assert d == "pic-P1" and dec.decode(REP) is d and dec.flush() == []


def test_decoder_with_defer_output_keeps_the_order():
    st = _Stubs()
    dec = SequenceDecoder(st.i, st.p, 32, 48, False, defer_output=True)
    stream = [FramePacket(True, 30, 0, b"I0"), REP, FramePacket(False, 31, 0, b"P1"), REP, REP, FramePacket(False, 31, 0, b"P2"),
              FramePacket(False, 31, 0, b"P3"), REP, FramePacket(True, 30, 0, b"I4"), REP]
    out = []
    for pkt in stream:
        got = dec.decode(pkt)
        assert isinstance(got, list)
        out += got
    out += dec.flush()
    assert out == ["pic-I0", "pic-I0", "pic-P1", "pic-P1", "pic-P1", "pic-P2", "pic-P3", "pic-P3", "pic-I4", "pic-I4"]
    assert dec.frame_idx == len(stream)
    dec = SequenceDecoder(st.i, st.p, 32, 48, False, defer_output=True)
    assert dec.decode(stream[0]) == ["pic-I0"] and dec.decode(stream[2]) == []
    assert dec.decode(REP) == ["pic-P1", "pic-P1"]                          # the pending picture first, as an I frame finishes it


def test_stream_decoder_keeps_the_resampled_picture_and_moves_the_grain(monkeypatch):
    import torch
    from opendcvc_amd import grain as G
    from opendcvc_amd import resize

    calls = []

    class Net:
        def set_curr_poc(self, poc):
            pass

        def clear_dpb(self):
            pass

        def add_ref_frame(self, feature, frame):
            pass

        def decompress(self, bit_stream, sps, qp, defer_output=False):
            calls.append("decompress")
            return {"x_hat": torch.full((1, 3, sps["height"], sps["width"]), float(bit_stream[0]))}

    class Scaler:
        def resample(self, x, size, to, name):
            calls.append("resample")
            return torch.full((1, 3, *to), float(x[0, 0, 0, 0]))

    class Grainer:
        def apply(self, x, size, params, t):
            calls.append(("grain", t))
            return x + t

    f = io.BytesIO()
    w = B.StreamWriter(f, display=(64, 96, "bicubic"))
    for pkt in (_pkt(payload=b"\x07", grain=P1), REP, REP, _pkt(False, b"\x08"), REP):
        w.write_frame(32, 48, False, pkt)
    sd = pipeline.StreamDecoder(io.BytesIO(f.getvalue()), Net(), Net(), "cpu", scaler=Scaler(), grainer=Grainer())
    frames = [sd.next() for _ in range(5)]
    assert calls == ["decompress", "resample", ("grain", 0), ("grain", 1), ("grain", 2), "decompress", "resample", ("grain", 3),
                     ("grain", 4)]
    assert [fr.repeat for fr in frames] == [False, True, True, False, True]
    assert frames[1].x_hat is frames[0].x_hat and frames[2].x_hat is frames[0].x_hat and frames[4].x_hat is frames[3].x_hat
    assert [float(fr.shown[0, 0, 0, 0]) for fr in frames] == [7.0, 8.0, 9.0, 11.0, 12.0]       # the shown pictures differ
    assert all(fr.x_hat.shape == (1, 3, 64, 96) and fr.display == (64, 96, "bicubic") for fr in frames)
    assert "repeat" in pipeline.DecodedFrame.__dataclass_fields__ and pipeline.DecodedFrame(1, 1, {}, True, None, None, 0).repeat is False


# ---------------------------------------------------------------------------------- the harness's options
BASE = "--src a.yuv --width 64 --height 64 --frames 1".split()


def test_dup_kwargs_and_the_parser_spellings():
    assert harness.dup_kwargs({}) == {} == harness.dup_kwargs(dict(frame_dup=False, dup_tol=None))
    assert harness.dup_kwargs(dict(frame_dup=None, dup_tol=2.0)) == {}
    assert harness.dup_kwargs(dict(frame_dup=True, dup_tol=None, other=1)) == {"frame_dup": True}
    assert harness.dup_kwargs(dict(frame_dup=True, dup_tol=0.0)) == {"frame_dup": True}
    assert harness.dup_kwargs(dict(frame_dup=True, dup_tol=1.5)) == {"frame_dup": True, "dup_tol": 1.5}
    ap = harness.build_parser()
    assert harness.dup_kwargs(vars(ap.parse_args(BASE))) == {}
    assert harness.dup_kwargs(vars(ap.parse_args(BASE + ["--frame-dup"]))) == {"frame_dup": True}
    assert harness.dup_kwargs(vars(ap.parse_args(BASE + "--frame_dup True --dup_tol 1.5".split()))) == {"frame_dup": True, "dup_tol": 1.5}
    assert harness.dup_kwargs(vars(ap.parse_args(BASE + "--frame-dup 0 --dup-tol 1.5".split()))) == {}
    opts, _ = harness.manifest_options(ap.parse_args("--test-config m.json --gpus 1 --gpu-ids 0 --frame-dup --dup-tol 2".split()), ap)
    assert opts["frame_dup"] is True and opts["dup_tol"] == 2.0
    opts, _ = harness.manifest_options(ap.parse_args("--test-config m.json --gpus 1 --gpu-ids 0".split()), ap)
    assert "frame_dup" not in opts and "dup_tol" not in opts
    params = inspect.signature(harness.run_one_point).parameters
    assert params["frame_dup"].default is False and params["dup_tol"].default == 0.0
    assert inspect.signature(harness._encode_pass).parameters["dup_tol"].default is None
    assert [n for n, _, _ in harness.POINT_OPTIONS][-1] == "film_grain"               # the table is not where it travels


def test_check_dup_and_run_one_points_argument_errors(tmp_path):
    harness.check_dup(False, 0.0)
    harness.check_dup(True, 0.0)
    harness.check_dup(True, 1.5)
    for frame_dup, tol in ((True, -1.0), (True, float("nan")), (False, -1.0)):
        with pytest.raises(ValueError, match="8-bit codes"):
            harness.check_dup(frame_dup, tol)
    with pytest.raises(ValueError, match="no effect"):
        harness.check_dup(False, 1.5)
    # before a net, a file or the device is touched
    for kw in (dict(dup_tol=1.0), dict(frame_dup=True, dup_tol=-2.0)):
        with pytest.raises(ValueError):
            harness.run_one_point(None, None, str(tmp_path / "missing.yuv"), 64, 64, 2, 32, **kw)


def test_dup_tol_without_frame_dup_is_a_usage_error(monkeypatch):
    monkeypatch.setattr(harness, "run_sweep", lambda *a, **kw: {})
    base = BASE + ["--out", os.devnull]
    harness.main(base + "--frame-dup --dup-tol 1.5".split())
    for extra in ("--dup-tol 1.5", "--frame-dup 0 --dup-tol 1.5", "--frame-dup --dup-tol -1"):
        with pytest.raises(SystemExit):
            harness.main(base + extra.split())


def test_without_frame_dup_run_one_point_gets_no_new_keyword(monkeypatch):
    seen = []
    monkeypatch.setattr(harness, "run_one_point", lambda *a, **kw: seen.append(kw) or {})
    monkeypatch.setattr(harness, "run_sweep", lambda *a, **kw: seen.append(kw) or {})
    job = dict(src_path="x.yuv", src_width=64, src_height=64, frame_num=2, qp_i=32, qp_p=32, intra_period=-1, reset_interval=32)
    base = BASE + ["--out", os.devnull]
    harness.run_job(("i", "p"), job, {})
    harness.main(base)
    harness.run_job(("i", "p"), job, {"frame_dup": True, "dup_tol": 1.0})
    harness.main(base + ["--frame-dup"])
    for kw in seen[:2]:
        assert "frame_dup" not in kw and "dup_tol" not in kw
    assert (seen[2]["frame_dup"], seen[2]["dup_tol"]) == (True, 1.0)
    assert seen[3]["frame_dup"] is True and "dup_tol" not in seen[3]


def test_run_one_point_hands_the_option_to_the_encode_pass(monkeypatch, tmp_path):
    class Stop(Exception):
        pass

    seen = []

    def encode_pass(*a, **kw):
        seen.append(kw)
        raise Stop

    class Net:
        rate_estimate = entropy = None

        def set_use_two_entropy_coders(self, two):
            pass

    monkeypatch.setattr(harness, "_encode_pass", encode_pass)
    for kw in (dict(frame_dup=True, dup_tol=1.5), dict(frame_dup=True), dict(frame_dup=False), {}):
        with pytest.raises(Stop):
            harness.run_one_point(Net(), Net(), str(tmp_path / "clip.yuv"), 64, 64, 2, 32, **kw)
    assert seen == [{"dup_tol": 1.5}, {"dup_tol": 0.0}, {}, {}]              # off: the call of before the option


# ---------------------------------------------------------------------------------- the C entry's argument errors
# a 64-byte-aligned host buffer stands in for every pointer: each call below must be refused before anything is launched
_BUF = ctypes.create_string_buffer(65536 + 64)
_PTR = (ctypes.addressof(_BUF) + 63) & ~63
_A, _B, _WS, _OUT = _PTR, _PTR + 24576, _PTR + 49152, _PTR + 49152 + 64          # a frame of 3 * 32 * 48 fp16 elements: 9216 bytes


def _maxdiff(dtype=_lib.F16, a=_A, b=_B, Hp=32, Wp=48, H=30, W=40, ws=_WS, out=_OUT):
    return _lib.lib().dcvc_frame_maxdiff(dtype, a, b, Hp, Wp, H, W, ws, out, None)


BAD = [dict(dtype=_lib.U8), dict(dtype=-1), dict(a=None), dict(b=None), dict(a=_A + 1), dict(b=_B + 1), dict(H=0), dict(W=0),
       dict(H=-3), dict(W=-1), dict(Hp=8), dict(Wp=8), dict(Hp=1 << 20, Wp=1 << 20), dict(ws=None), dict(ws=_WS + 2), dict(out=None),
       dict(out=_OUT + 2), dict(a=_A, b=_A, H=0), dict(dtype=_lib.F32, a=_A + 2), dict(dtype=_lib.F32, b=_B + 2)]


@pytest.mark.parametrize("kw", BAD, ids=lambda kw: "-".join(kw))
def test_a_bad_argument_is_refused_by_name_before_any_launch(kw):
    before = bytes(_BUF)
    assert _maxdiff(**kw) == -1, kw
    err = _lib.lib().dcvc_last_error()
    assert b"dcvc_frame_maxdiff" in err, err
    assert bytes(_BUF) == before


def test_ws_bytes_and_exports():
    assert _lib.lib().dcvc_frame_maxdiff_ws_bytes() == 32
    assert "dcvc_frame_maxdiff" in _lib.EXPORTS and "dcvc_frame_maxdiff_ws_bytes" in _lib.EXPORTS
    assert repeat.RepeatDetector and pipeline.REPEAT is not None
