"""The harness's single spellings, on the host: the per-point option table against run_one_point's signature and the command
line, StreamReader.read_packet against read_frame, and pipeline.StreamDecoder's off path with stub codecs.  No GPU."""
import inspect
import io

import pytest
import torch

from opendcvc_amd import bitstream as B
from opendcvc_amd import grain, harness, pipeline, resize
from opendcvc_amd.grain import GrainParams
from opendcvc_amd.pipeline import FramePacket

# --verbose is the one option whose command-line default is not run_one_point's: the command line reports frame times unless
# told otherwise, a caller of run_one_point / run_job asks for them
CLI_DEFAULTS_OF_THEIR_OWN = {"verbose": 1}


# ---------------------------------------------------------------------------------- the option table
def test_point_kwargs_of_nothing_are_the_signatures_defaults():
    params = inspect.signature(harness.run_one_point).parameters
    names = [name for name, _, _ in harness.POINT_OPTIONS]
    assert names == ["verbose", "verbose_json", "calc_ssim", "metrics", "entropy", "scenecut", "min_keyint", "digest",
                     "coded_size", "scale_filter", "film_grain"]
    got = harness.point_kwargs({})
    assert list(got) == names
    for name, default, _ in harness.POINT_OPTIONS:
        assert name in params, name
        assert params[name].default == default and type(params[name].default) is type(default), name
        assert got[name] == default and type(got[name]) is type(default), name
    # set values pass, None and a missing key mean the default
    opts = dict(verbose=2, verbose_json=True, calc_ssim=1, metrics="device", entropy="device", scenecut=150, min_keyint=2,
                digest=1, coded_size=(64, 80), scale_filter="bicubic", film_grain="auto")
    want = dict(opts, calc_ssim=True, digest=True)
    assert harness.point_kwargs(opts) == want and harness.point_kwargs(dict(opts, unrelated=3)) == want
    assert harness.point_kwargs(dict.fromkeys(names)) == got


def test_every_command_line_option_of_the_table_has_the_tables_default():
    ap = harness.build_parser()
    offered = {a.dest: a for a in ap._actions}
    for name, default, _ in harness.POINT_OPTIONS:
        assert name in offered, f"--{name}: not on the command line"
        want = CLI_DEFAULTS_OF_THEIR_OWN.get(name, default)
        assert ap.get_default(name) == want and type(ap.get_default(name)) is type(want), name
    args = ap.parse_args("--src a.yuv --width 64 --height 64 --frames 1".split())
    assert harness.point_kwargs(vars(args)) == dict(harness.point_kwargs({}), **CLI_DEFAULTS_OF_THEIR_OWN)
    args = ap.parse_args("--test-config m.json --gpus 1 --gpu-ids 0 --film-grain --digest --coded-size 80x64 --verbose 0".split())
    kw = harness.point_kwargs(vars(args))
    assert (kw["film_grain"], kw["digest"], kw["coded_size"], kw["verbose"]) == ("auto", True, (64, 80), 0)
    opts, _ = harness.manifest_options(args, ap)
    assert {k: opts[k] for k in kw} == kw                          # the pool's options carry the same values


def test_run_job_and_main_hand_on_the_same_keywords(monkeypatch):
    seen = []
    monkeypatch.setattr(harness, "run_one_point", lambda *a, **kw: seen.append(kw) or {})
    monkeypatch.setattr(harness, "run_sweep", lambda *a, **kw: seen.append(kw) or {})
    job = dict(src_path="x.yuv", src_width=64, src_height=64, frame_num=2, qp_i=32, qp_p=32, intra_period=-1, reset_interval=32)
    harness.run_job(("i", "p"), job, {})
    assert {k: seen[0][k] for k in harness.point_kwargs({})} == harness.point_kwargs({})
    assert seen[0]["target_bpp"] is None and seen[0]["src_type"] == "yuv420" and seen[0]["device"] == "cuda:0"
    import os
    harness.main(f"--src a.yuv --width 64 --height 64 --frames 1 --scenecut 150 --entropy device --out {os.devnull}".split())
    want = dict(harness.point_kwargs({}), scenecut=150, entropy="device", **CLI_DEFAULTS_OF_THEIR_OWN)
    assert {k: seen[1][k] for k in want} == want and seen[1]["target_bpp"] is None


# ---------------------------------------------------------------------------------- StreamReader.read_packet
P1 = GrainParams(513, 1, (1, 2, 3, 4, 5, 6, 7, 8), 9, 10)


def _hand_written_stream():
    """SPS, display, grain, digest, chunked and plain units, written unit by unit: two SPS (the second without a display
    unit), grain switched on, replaced and off"""
    f = io.BytesIO()
    sps0 = dict(sps_id=0, height=64, width=80, use_ada_i=0, ec_part=0)
    sps1 = dict(sps_id=1, height=64, width=80, use_ada_i=1, ec_part=1)
    B.write_sps(f, sps0)
    B.write_display(f, 0, 96, 128, "bicubic")
    B.write_grain(f, 0, P1)
    B.write_digest(f, 0, 0x0123456789ABCDEF)
    B.write_ip(f, True, 0, 30, b"\x01" * 10)                      # 0: I, display, grain, digest
    B.write_ip(f, False, 0, 31, b"\x02" * 200, chunked=True)      # 1: P chunked, no digest
    B.write_sps(f, sps1)
    B.write_digest(f, 1, 7)
    B.write_ip(f, False, 1, 33, b"\x03" * 20000)                  # 2: P under the second SPS (no display unit), digest
    B.write_grain(f, 0, GrainParams(seed=3))                      # all strengths 0: grain off
    B.write_ip(f, True, 0, 29, b"", chunked=True)                 # 3: I chunked, empty payload
    B.write_ip(f, False, 0, 35, b"\x05")                          # 4: plain P
    return f.getvalue()


def test_read_packet_is_read_frame_plus_the_attributes():
    data = _hand_written_stream()
    a, b = B.StreamReader(io.BytesIO(data)), B.StreamReader(io.BytesIO(data))
    seen = []
    for _ in range(5):
        sps, is_i, qp, payload = a.read_frame()
        sps_b, pkt = b.read_packet()
        assert isinstance(pkt, FramePacket) and sps_b == sps
        assert (pkt.is_i, pkt.qp, pkt.use_ada_i, pkt.bit_stream, pkt.chunked, pkt.digest, pkt.grain) == \
            (is_i, qp, sps["use_ada_i"], payload, a.chunked, a.digest, None)
        assert (b.chunked, b.digest, b.display, b.grain, b.grain_t) == (a.chunked, a.digest, a.display, a.grain, a.grain_t)
        seen.append((sps["sps_id"], is_i, qp, len(payload), pkt.chunked, pkt.digest, b.display, b.grain, b.grain_t))
    assert seen == [(0, True, 30, 10, False, 0x0123456789ABCDEF, (96, 128, "bicubic"), P1, 0),
                    (0, False, 31, 200, True, None, (96, 128, "bicubic"), P1, 1),
                    (1, False, 33, 20000, False, 7, None, P1, 2),
                    (0, True, 29, 0, True, None, (96, 128, "bicubic"), None, 0),
                    (0, False, 35, 1, False, None, (96, 128, "bicubic"), None, 1)]
    for rd in (a, b):
        with pytest.raises(EOFError):
            rd.read_packet()


# ---------------------------------------------------------------------------------- StreamDecoder with stub codecs
class _Net:
    """a codec that decodes a payload into a picture of the payload's first byte; CPU tensors, every call recorded"""

    def __init__(self, calls):
        self.calls = calls

    def set_curr_poc(self, poc):
        self.calls.append(("set_curr_poc", poc))

    def clear_dpb(self):
        self.calls.append("clear_dpb")

    def add_ref_frame(self, feature, frame):
        self.calls.append("add_ref_frame")

    def reset_ref_feature(self):
        self.calls.append("reset_ref_feature")

    def decompress(self, bit_stream, sps, qp, defer_output=False):
        self.calls.append(("decompress", sps["height"], sps["width"], sps["ec_part"], qp))
        return {"x_hat": torch.full((1, 3, sps["height"], sps["width"]), float(bit_stream[0]))}


def test_stream_decoder_without_extension_units_launches_nothing_of_them(monkeypatch):
    def refuse(*a, **kw):
        raise AssertionError("constructed on the off path")
    monkeypatch.setattr(resize, "Resampler", refuse)
    monkeypatch.setattr(grain, "FilmGrain", refuse)
    f = io.BytesIO()
    w = B.StreamWriter(f)
    pkts = [FramePacket(True, 30, 0, b"\x07abc"), FramePacket(False, 31, 1, b"\x08"), FramePacket(False, 32, 0, b"\x09" * 300)]
    for p in pkts:
        w.write_frame(32, 48, False, p)
    w.write_frame(16, 16, True, FramePacket(True, 33, 0, b"\x0a"))          # another SPS: the decoder follows it
    i_calls, p_calls = [], []
    sd = pipeline.StreamDecoder(io.BytesIO(f.getvalue()), _Net(i_calls), _Net(p_calls), "cpu")
    assert sd.digests_checked == 0 and sd.dec is None
    sd.check_digests()
    frames = [sd.next() for _ in range(4)]
    for fr, value, (h, w_), is_i in zip(frames, (7, 8, 9, 10), [(32, 48)] * 3 + [(16, 16)], (True, False, False, True)):
        assert isinstance(fr, pipeline.DecodedFrame) and fr.shown is fr.x_hat
        assert fr.x_hat.shape == (1, 3, h, w_) and float(fr.x_hat[0, 0, 0, 0]) == value
        assert (fr.sps["height"], fr.sps["width"], fr.is_i, fr.display, fr.grain) == (h, w_, is_i, None, None)
    assert [fr.grain_t for fr in frames] == [1, 2, 3, 4]
    assert sd.scaler is None and sd.grainer is None and sd.digests_checked == 0
    assert i_calls == [("decompress", 32, 48, 0, 30), ("decompress", 16, 16, 1, 33)]
    assert p_calls == [("set_curr_poc", 0), "clear_dpb", "add_ref_frame", "reset_ref_feature", ("decompress", 32, 48, 0, 31),
                       ("decompress", 32, 48, 0, 32), "clear_dpb", "add_ref_frame"]
    sd.check_digests()
    sd.flush()
    with pytest.raises(EOFError):
        sd.next()
