"""Repeated-frame coding on the GPU (docs/frame_repeat.md): dcvc_frame_maxdiff of csrc/dcvc_repeat.hip against the numpy
restatement (tests/repeat_ref.py) word for word, in fp16 and fp32, repeat.RepeatDetector's rule, and the option end to end
through the harness, the container's repeat unit, pipeline.StreamDecoder and the two-stage pipeline."""
import ctypes
import io

import numpy as np
import pytest
import torch

import repeat_ref as R
from opendcvc_amd import _lib, harness, repeat, weights
from opendcvc_amd.bitstream import StreamReader
from opendcvc_amd.entropy import PinnedBuffer
from opendcvc_amd.grain import GrainParams
from opendcvc_amd.repeat import RepeatDetector

pytestmark = pytest.mark.gpu

DTYPES = [pytest.param(torch.float32, np.float32, id="fp32"), pytest.param(torch.float16, np.float16, id="fp16")]
NAN_KEY = 0x7FC00000
# (H, W, Hp, Wp): padding on both sides; a last tile cut both ways; rows of 100 (16-byte rows in fp32 only); smaller than a
# tile; many workgroups (2 x 9 x 3 tiles of 256 x 32)
SHAPES = [(40, 72, 48, 80), (70, 98, 80, 112), (70, 98, 72, 100), (17, 33, 32, 48), (270, 480, 272, 480)]


def _dev(host, offset=0):
    """the host frame [3][Hp][Wp] on the device as [1, 3, Hp, Wp]; offset: that many elements into a larger allocation"""
    t = torch.from_numpy(np.array(host))
    if not offset:
        return t[None].cuda()
    flat = torch.empty(host.size + 16, dtype=t.dtype, device="cuda")
    dev = flat[offset:offset + host.size].view(1, *host.shape)
    dev.copy_(t[None])
    assert dev.data_ptr() % 16 == (offset * host.itemsize) % 16 and dev.is_contiguous()
    return dev


def _frame(ndt, H, W, Hp, Wp, seed, poison=(np.nan, 6e4)):
    """uniform content in [0, 1) in a frame whose padding holds the poison values, alternating"""
    host = np.empty((3, Hp, Wp), ndt)
    host[:, ::2], host[:, 1::2] = poison
    host[:, :H, :W] = np.random.default_rng(seed).random((3, H, W), dtype=np.float32).astype(ndt)
    return host


class _Compare:
    """one workspace, zeroed once, and two pinned result slots: call() enqueues a compare, read() waits and returns the words"""

    def __init__(self):
        self.lib = _lib.lib()
        assert self.lib.dcvc_frame_maxdiff_ws_bytes() == 32
        self.ws = torch.zeros(32, dtype=torch.uint8, device="cuda")
        self.pinned = PinnedBuffer(32)
        self.words = self.pinned.view(np.uint32, 8)

    def call(self, a, b, H, W, slot=0):
        assert a.shape == b.shape and a.dtype == b.dtype
        self.words[4 * slot:4 * slot + 4] = 0xFFFFFFFF
        rc = self.lib.dcvc_frame_maxdiff(0 if a.dtype == torch.float16 else 1, ctypes.c_void_p(a.data_ptr()),
                                         ctypes.c_void_p(b.data_ptr()), a.shape[2], a.shape[3], H, W,
                                         ctypes.c_void_p(self.ws.data_ptr()), ctypes.c_void_p(self.pinned.ptr + 16 * slot),
                                         ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, self.lib.dcvc_last_error()

    def read(self, slot=0):
        torch.cuda.synchronize()
        return self.words[4 * slot:4 * slot + 4].copy()

    def run(self, a, b, H, W):
        self.call(a, b, H, W)
        return self.read()

    def ws_words(self):
        torch.cuda.synchronize()
        return self.ws.cpu().numpy().view(np.uint32).tolist()


@pytest.fixture(scope="module")
def cmp():
    return _Compare()


def _same(got, want, what):
    print(f"{what}: kernel {[hex(v) for v in got]}, restatement {[hex(v) for v in want]}")
    assert got.dtype == want.dtype == np.uint32 and np.array_equal(got, want), what


# ---------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("tdt,ndt", DTYPES)
@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("H,W,Hp,Wp", SHAPES)
def test_maxdiff_equals_the_restatement(cmp, H, W, Hp, Wp, offset, tdt, ndt):
    seed = H * 1000 + W
    # the two frames' padding holds NaN where the other's holds 6e4: a padding sample read would be a NaN key
    a, b = _frame(ndt, H, W, Hp, Wp, seed), _frame(ndt, H, W, Hp, Wp, seed + 1, poison=(6e4, np.nan))
    da = _dev(a, offset)
    want = R.maxdiff(a, b, H, W)
    assert all(0 < k < 0x3F800000 for k in want[:3])
    _same(cmp.run(da, _dev(b, offset), H, W), want, "random frames")
    if offset:                                             # one aligned address does not allow the 16-byte form
        _same(cmp.run(_dev(a), _dev(b, offset), H, W), want, "random frames, only the second one off")
        _same(cmp.run(da, _dev(b), H, W), want, "random frames, only the first one off")

    same = _frame(ndt, H, W, Hp, Wp, seed, poison=(6e4, np.nan))              # a's picture in b's padding
    _same(cmp.run(da, _dev(same, offset), H, W), np.zeros(4, np.uint32), "identical pictures")

    for p in range(3):                                     # one sample: each corner, the last one is the plane's last valid sample
        for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):
            one = same.copy()
            one[p, y, x] = ndt(float(one[p, y, x]) + 0.25 + 0.125 * p)
            want = R.maxdiff(a, one, H, W)
            assert want[p] > 0 and sum(want) == want[p]
            _same(cmp.run(da, _dev(one, offset), H, W), want, f"one sample of plane {p} at ({y}, {x})")

    zero, minus = a.copy(), same.copy()
    zero[:, :H, :W], minus[:, :H, :W] = 0.0, -0.0
    assert np.signbit(minus[0, 0, 0]) and not np.signbit(zero[0, 0, 0])
    _same(cmp.run(_dev(zero, offset), _dev(minus, offset), H, W), np.zeros(4, np.uint32), "+0 against -0")

    bad = same.copy()
    bad[1, H // 2, W // 2] = np.nan
    bad[2, H - 1, W // 3] = np.inf
    bad_a = a.copy()
    bad_a[2, H - 1, W // 3] = np.inf                       # inf - inf
    want = R.maxdiff(bad_a, bad, H, W)
    assert want.tolist() == [0, NAN_KEY, NAN_KEY, 0]
    _same(cmp.run(_dev(bad_a, offset), _dev(bad, offset), H, W), want, "a NaN and inf - inf")
    bad_a[0, 0, W - 1] = -np.inf                           # -inf against a finite sample: the key of +inf
    want = R.maxdiff(bad_a, bad, H, W)
    assert want[0] == 0x7F800000
    _same(cmp.run(_dev(bad_a, offset), _dev(bad, offset), H, W), want, "an infinite difference")

    # two compares in a row on one workspace, nothing in between: the first one left it ready
    c = _frame(ndt, H, W, Hp, Wp, seed + 2)
    db, dc = _dev(b, offset), _dev(c, offset)
    cmp.call(da, db, H, W, slot=0)
    cmp.call(dc, da, H, W, slot=1)
    _same(cmp.read(0), R.maxdiff(a, b, H, W), "first of two compares")
    _same(cmp.read(1), R.maxdiff(c, a, H, W), "second of two compares")

    _same(cmp.run(da, da, H, W), np.zeros(4, np.uint32), "a frame against itself")
    dbad = _dev(bad, offset)
    _same(cmp.run(dbad, dbad, H, W), np.array([0, NAN_KEY, NAN_KEY, 0], np.uint32), "a frame with a NaN and an inf against itself")
    assert not any(cmp.ws_words())                        # ready for the next call


# ---------------------------------------------------------------------------------- the detector
@pytest.mark.parametrize("tdt,ndt", DTYPES)
def test_detector_compares_with_the_last_frame_that_was_no_repeat(tdt, ndt):
    H, W, Hp, Wp = 40, 72, 48, 80
    det = RepeatDetector("cuda:0", 2.0)
    t = np.float32(2.0) / np.float32(255.0)
    assert det.tol == t and det.maxima() is None and det.repeats == 0
    base = np.zeros((3, Hp, Wp), ndt)
    base[:, :H, :W] = 0.5

    def stepped(step):
        x = base.copy()
        x[1, H - 1, W - 1] = ndt(0.5 + step)
        return _dev(x), float(np.abs(np.float32(x[1, H - 1, W - 1]) - np.float32(0.5)))

    x0 = _dev(base)
    assert det.is_repeat(x0, (H, W)) is False and det.maxima() is None         # the first frame: nothing is compared
    x1, d1 = stepped(0.6 * t)
    assert d1 <= t and det.is_repeat(x1, (H, W)) is True and det.maxima() == (0.0, d1, 0.0) and det.repeats == 1
    x2, d2 = stepped(1.2 * t)                              # 0.6 t from the frame before, 1.2 t from the reference: a ramp does not pass
    assert d2 > t and det.is_repeat(x2, (H, W)) is False and det.maxima() == (0.0, d2, 0.0) and det.repeats == 1
    assert det.is_repeat(x1, (H, W)) is True and det.repeats == 2              # x2 is the reference now
    assert det.is_repeat(x0, (H, W)) is False and det.is_repeat(x0, (H, W)) is True
    assert det.is_repeat(x0, (H - 2, W)) is False and det.maxima() == (0.0, 0.0, 0.0)      # another size: no compare, no repeat
    assert det.is_repeat(x0, (H - 2, W)) is True and det.repeats == 4
    bad = base.copy()
    bad[0, 1, 1] = np.nan
    xb = _dev(bad)
    assert det.is_repeat(xb, (H - 2, W)) is False and det.is_repeat(xb, (H - 2, W)) is False and np.isnan(det.maxima()[0])
    with pytest.raises(ValueError):
        RepeatDetector("cuda:0", -1.0)
    with pytest.raises(ValueError):
        RepeatDetector("cuda:0", float("nan"))


def test_detector_at_the_exact_edge_of_the_tolerance():
    H, W = 17, 33
    t = np.float32(2.0) / np.float32(255.0)
    a = np.zeros((3, 32, 48), np.float32)
    for value, want in ((t, True), (np.nextafter(t, np.float32(1.0)), False), (np.nextafter(t, np.float32(0.0)), True)):
        b = a.copy()
        b[2, 16, 32] = value                               # against 0: the difference IS the sample
        det = RepeatDetector("cuda:0", 2.0)
        assert det.is_repeat(_dev(a), (H, W)) is False
        assert det.is_repeat(_dev(b), (H, W)) is want and det.maxima() == (0.0, 0.0, float(value))
    det = RepeatDetector("cuda:0", 0.0)
    assert not det.is_repeat(_dev(a), (H, W)) and det.is_repeat(_dev(a), (H, W))
    b = a.copy()
    b[0, 0, 0] = np.float32(1e-45)                         # the smallest fp32 there is
    assert det.is_repeat(_dev(b), (H, W)) is False and det.maxima() == (float(np.float32(1e-45)), 0.0, 0.0)


# ---------------------------------------------------------------------------------- end to end
H, W = 128, 160
PARAMS = GrainParams(4242, 1, (8, 40, 72, 104, 136, 168, 200, 255), 90, 160)


def _make_nets():
    from opendcvc_amd.models import DMC, DMCI
    out = []
    for cls, name in ((DMCI, "dmci"), (DMC, "dmc")):
        m = cls()
        m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in weights.make_state_dict(name, 1234).items()})
        m.to("cuda").eval()
        m.update(0.12)
        out.append(m)
    return out


@pytest.fixture(scope="module")
def nets():
    return _make_nets()


def _content(i, h=H, w=W):
    return [p.copy() for p in weights.synthetic_frame_yuv420(h, w, i, 3)]


def _write(path, frames):
    with open(path, "wb") as f:
        for planes in frames:
            for plane in planes:
                f.write(np.ascontiguousarray(plane, np.uint8).tobytes())
    return str(path)


def _units(data, n):
    """the n frames of a container -> (is_i, qp, payload, repeat, digest is there) each"""
    rd = StreamReader(io.BytesIO(data))
    out = []
    for _ in range(n):
        sps, is_i, qp, payload = rd.read_frame()
        out.append((is_i, qp, payload, rd.repeat, rd.digest is not None))
    return out


def _frames_of_file(data, h=H, w=W):
    n = h * w * 3 // 2
    assert len(data) % n == 0
    return [data[i:i + n] for i in range(0, len(data), n)]


def test_the_coded_frames_are_those_of_the_clip_without_its_repeats(nets, tmp_path):
    A, Bf, C = _content(0), _content(1), _content(2)
    pattern = [0, 1, 0, 1, 1, 0]
    dup = _write(tmp_path / "dup.yuv", [A, A, Bf, Bf, Bf, C])
    plain = _write(tmp_path / "plain.yuv", [A, Bf, C])
    kw = dict(intra_period=2, verbose_json=True)
    log = harness.run_one_point(*nets, dup, W, H, 6, 32, 32, frame_dup=True, bin_path=str(tmp_path / "dup.bin"),
                                rec_path=str(tmp_path / "dup_rec.yuv"), **kw)
    ref = harness.run_one_point(*nets, plain, W, H, 3, 32, 32, bin_path=str(tmp_path / "plain.bin"),
                                rec_path=str(tmp_path / "plain_rec.yuv"), **kw)
    assert log["repeat_frames"] == 3 and log["dup_tol"] == 0.0 and log["frame_repeat"] == pattern
    assert list(log)[-3:] == ["repeat_frames", "dup_tol", "frame_repeat"] and list(log)[:-3] == list(ref)
    assert len(log["frame_type"]) == 6 and log["frame_type"] == [0, 1, 1, 1, 1, 0]          # a repeat counts as a P frame
    assert (log["i_frame_num"], log["p_frame_num"]) == (2, 4) and ref["frame_type"] == [0, 1, 0]
    data, plain_data = open(tmp_path / "dup.bin", "rb").read(), open(tmp_path / "plain.bin", "rb").read()
    units, want = _units(data, 6), _units(plain_data, 3)
    assert [u[3] for u in units] == [bool(r) for r in pattern]
    assert [u for u in units if not u[3]] == want                               # every I / P payload, byte for byte
    assert len(data) == len(plain_data) + 3                                     # three one-byte units, nothing else
    assert [round(b * H * W) for b in log["frame_bpp"]] == [round(ref["frame_bpp"][0] * H * W), 8,
                                                            round(ref["frame_bpp"][1] * H * W), 8, 8,
                                                            round(ref["frame_bpp"][2] * H * W)]
    assert round(sum(log["frame_bpp"]) * H * W) == 8 * len(data)
    rec = _frames_of_file(open(tmp_path / "dup_rec.yuv", "rb").read())
    plain_rec = _frames_of_file(open(tmp_path / "plain_rec.yuv", "rb").read())
    assert len(rec) == 6 and rec == [plain_rec[0]] * 2 + [plain_rec[1]] * 3 + [plain_rec[2]]       # bit for bit
    for i, j in enumerate((0, 0, 1, 1, 1, 2)):                                  # each picture against its own source frame
        assert log["frame_psnr"][i] == ref["frame_psnr"][j]


def test_a_ramp_below_the_tolerance_does_not_drift(nets, tmp_path):
    base = [np.minimum(p, 250) for p in _content(0)]
    ramp = _write(tmp_path / "ramp.yuv", [[p + k for p in base] for k in range(4)])
    kw = dict(intra_period=-1, verbose_json=True)
    log = harness.run_one_point(*nets, ramp, W, H, 4, 32, 32, frame_dup=True, dup_tol=1.5, **kw)
    assert log["frame_repeat"] == [0, 1, 0, 1] and log["repeat_frames"] == 2 and log["dup_tol"] == 1.5
    log = harness.run_one_point(*nets, ramp, W, H, 4, 32, 32, frame_dup=True, dup_tol=0.0, **kw)
    assert log["frame_repeat"] == [0, 0, 0, 0] and log["repeat_frames"] == 0


def _barred(planes, bar=32):
    out = []
    for k, plane in enumerate(planes):
        b = bar if k == 0 else bar // 2
        full = np.full((plane.shape[0] + 2 * b, plane.shape[1]), 16 if k == 0 else 128, np.uint8)
        full[b:b + plane.shape[0]] = plane
        out.append(full)
    return out


def test_frame_dup_with_the_other_extensions(nets, tmp_path):
    """Every extension at once.  Rate control hands the budget a repeat frees to its neighbours (RateController.skip), so with
    target_bpp the qp trace - and with it the payloads - is NOT that of the clip without the repeats: the payloads are held
    against that clip with every other option on, and the run with target_bpp on top is checked for everything else."""
    from opendcvc_amd.pipeline import StreamDecoder
    frames = [_barred(_content(i, H - 64, W)) for i in range(5)]              # 64 x 160 of content under 32-row bars
    order = [0, 0, 1, 2, 2, 2, 3, 4]
    pattern = [0, 1, 0, 0, 1, 1, 0, 0]
    dup = _write(tmp_path / "dup.yuv", [frames[i] for i in order])
    plain = _write(tmp_path / "plain.yuv", frames)
    kw = dict(intra_period=4, digest=True, film_grain=PARAMS, coded_size=(48, 96), crop="auto", temporal_filter=1, scenecut=150,
              lookahead=2, verbose_json=True)
    log = harness.run_one_point(*nets, dup, W, H, 8, 32, 32, frame_dup=True, bin_path=str(tmp_path / "dup.bin"), **kw)
    ref = harness.run_one_point(*nets, plain, W, H, 5, 32, 32, bin_path=str(tmp_path / "plain.bin"), **kw)
    assert log["frame_repeat"] == pattern and log["repeat_frames"] == 3
    assert log["digests_checked"] == 5 == ref["digests_checked"]               # the coded frames
    assert log["active_area"] == [32, 32, 0, 0] and (log["coded_height"], log["coded_width"]) == (48, 96)
    assert log["scene_cuts"] == ref["scene_cuts"] and log["tf_mean_weight"] == ref["tf_mean_weight"]
    data = open(tmp_path / "dup.bin", "rb").read()
    units, want = _units(data, 8), _units(open(tmp_path / "plain.bin", "rb").read(), 5)
    assert [u[3] for u in units] == [bool(r) for r in pattern]
    assert [u for u in units if not u[3]] == want and all(u[4] for u in want)
    assert not any(u[4] for u in units if u[3])                                # no digest unit in front of a repeat

    rate = harness.run_one_point(*nets, dup, W, H, 8, 32, 32, frame_dup=True, target_bpp=0.5, bin_path=str(tmp_path / "rate.bin"),
                                 **kw)
    assert rate["frame_repeat"] == pattern and rate["digests_checked"] == 5 and len(rate["frame_rc_qp"]) == 8
    assert [rate["frame_rc_qp"][i] for i in (1, 4, 5)] == [rate["frame_rc_qp"][i] for i in (0, 3, 3)]       # the last qp again
    assert [round(rate["frame_rc_est_bpp"][i] * H * W) for i in (1, 4, 5)] == [8, 8, 8]
    assert [round(rate["frame_bpp"][i] * H * W) for i in (1, 4, 5)] == [8, 8, 8]

    for name in ("dup.bin", "rate.bin"):
        with open(tmp_path / name, "rb") as f:
            decoder = StreamDecoder(f, *nets, "cuda:0")
            got = []
            for _ in range(8):
                fr = decoder.next()
                assert fr.grain == PARAMS and fr.active.extents == [32, 32, 0, 0] and fr.display == (H - 64, W, "lanczos3")
                assert fr.x_hat.shape == fr.shown.shape == (1, 3, H, W) and fr.shown is not fr.x_hat
                got.append((fr.repeat, fr.grain_t, fr.x_hat.clone(), fr.shown.clone()))
            decoder.flush()
            assert decoder.digests_checked == 5
        assert [g[0] for g in got] == [bool(r) for r in pattern]
        for i in (1, 4, 5):                                                     # the same picture, the grain moves on
            assert torch.equal(got[i][2], got[i - 1][2]) and not torch.equal(got[i][3], got[i - 1][3])
            assert got[i][1] == got[i - 1][1] + 1
        assert not torch.equal(got[3][2], got[2][2])


def test_repeat_packets_through_the_device_coder_and_the_two_stage_pipeline(nets, tmp_path):
    from opendcvc_amd.pipeline import (REPEAT, EncodeDecodePipeline, FramePacket, SequenceDecoder, SequenceEncoder,
                                       load_yuv420_frame)
    dec_nets = _make_nets()
    for m in list(nets) + dec_nets:
        m.set_use_two_entropy_coders(False)
        m.entropy = "device"
        m.rate_estimate = False
    try:
        xs = [load_yuv420_frame(*(torch.from_numpy(p).cuda() for p in _content(i)), torch.float32) for i in range(3)]
        torch.cuda.synchronize()
        clip = [xs[0], REPEAT, xs[1], REPEAT, REPEAT, xs[2]]
        pattern = [False, True, False, True, True, False]
        plain = SequenceEncoder(*nets, 32, intra_period=2)
        want = [plain.encode(x) for x in xs]
        assert all(p.chunked for p in want) and [p.is_i for p in want] == [True, False, True]
        for defer in (False, True):
            enc = SequenceEncoder(*nets, 32, intra_period=2, defer_stream=defer)
            dec = SequenceDecoder(*dec_nets, H, W, False, defer_output=defer)
            pkts, pics = [], []
            EncodeDecodePipeline(enc, dec, torch.device("cuda", 0)).run(clip, on_packet=pkts.append,
                                                                        on_frame=lambda t: pics.append((t, t.float().cpu().numpy())))
            assert [p.repeat for p in pkts] == pattern, defer                    # in order
            assert [p for p in pkts if not p.repeat] == want
            assert all(p == FramePacket(False, 0, 0, b"", repeat=True) for p in pkts if p.repeat)
            assert len(pics) == 6 and dec.frame_idx == 6 and enc.frame_idx == 3
            for i in (1, 3, 4):
                assert pics[i][0] is pics[i - 1][0] and np.array_equal(pics[i][1], pics[i - 1][1])      # the same tensor
            assert not np.array_equal(pics[2][1], pics[0][1]) and not np.array_equal(pics[5][1], pics[2][1])
    finally:
        for m in nets:
            m.entropy = "host"
    # the harness with the device coder: chunked frame units and repeat units side by side
    A, Bf = _content(0), _content(1)
    dup = _write(tmp_path / "dup.yuv", [A, A, Bf, Bf])
    log = harness.run_one_point(*nets, dup, W, H, 4, 32, 32, frame_dup=True, entropy="device", digest=True, verbose_json=True,
                                bin_path=str(tmp_path / "dev.bin"))
    assert log["frame_repeat"] == [0, 1, 0, 1] and log["digests_checked"] == 2
    rd = StreamReader(io.BytesIO(open(tmp_path / "dev.bin", "rb").read()))
    seen = []
    for _ in range(4):
        rd.read_frame()
        seen.append((rd.repeat, rd.chunked))
    assert seen == [(False, True), (True, False), (False, True), (True, False)]


def test_off_is_off_and_a_clip_without_repeats_is_coded_as_ever(nets, tmp_path, monkeypatch):
    clip = _write(tmp_path / "clip.yuv", [_content(i) for i in range(4)])
    kw = dict(intra_period=2, verbose_json=True)
    on = harness.run_one_point(*nets, clip, W, H, 4, 32, 32, frame_dup=True, bin_path=str(tmp_path / "on.bin"), **kw)

    def refuse(*a, **k):
        raise AssertionError("constructed on the off path")
    monkeypatch.setattr(repeat, "RepeatDetector", refuse)
    a = harness.run_one_point(*nets, clip, W, H, 4, 32, 32, bin_path=str(tmp_path / "a.bin"), **kw)
    b = harness.run_one_point(*nets, clip, W, H, 4, 32, 32, frame_dup=False, dup_tol=0.0, bin_path=str(tmp_path / "b.bin"), **kw)
    data = open(tmp_path / "a.bin", "rb").read()
    assert data == open(tmp_path / "b.bin", "rb").read()
    assert list(a) == list(b) and not {"repeat_frames", "dup_tol", "frame_repeat"} & set(a)
    # no frame repeats: the option finds nothing, writes no unit, and the stream is the one of the option off
    assert on["repeat_frames"] == 0 and on["frame_repeat"] == [0] * 4 and list(on)[:-3] == list(a)
    assert open(tmp_path / "on.bin", "rb").read() == data
    assert on["frame_bpp"] == a["frame_bpp"] and on["frame_psnr"] == a["frame_psnr"] and on["frame_type"] == a["frame_type"]
