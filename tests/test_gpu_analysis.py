"""Scene-cut detection on the device: dcvc_frame_analyze against its numpy restatement (tests/analysis_ref.py) bit for
bit, analysis.FrameAnalyzer over a sequence, and the adaptive I frames of pipeline.SequenceEncoder end to end - container,
decoder, deferred stream, two-stage pipeline and harness."""
import ctypes
import io

import numpy as np
import pytest
import torch

import analysis_ref as R
from opendcvc_amd import weights

pytestmark = pytest.mark.gpu

_NP = {torch.float16: np.float16, torch.float32: np.float32}


# ---------------------------------------------------------------------------------- the kernels
class _Caller:
    """the buffers one dcvc_frame_analyze call needs, allocated per case"""

    def __init__(self, h, w):
        from opendcvc_amd import _lib
        from opendcvc_amd.entropy import PinnedBuffer
        self.lib = _lib.lib()
        self.check = _lib.check
        self.h, self.w = h, w
        self.pinned = PinnedBuffer(32)
        self.words = self.pinned.view(np.uint64, 4)
        need = self.lib.dcvc_frame_analysis_ws_bytes(h, w)
        self.ws = torch.empty(max(int(need), 4096), dtype=torch.uint8, device="cuda")      # (a bad size has no need)

    def __call__(self, dtype, luma_ptr, ld, prev, out, check=True):
        from opendcvc_amd import nn as L
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        rc = self.lib.dcvc_frame_analyze(L.dtype_code(dtype), ctypes.c_void_p(luma_ptr), ld, self.h, self.w, L._p(prev),
                                         L._p(out), L._p(self.ws), ctypes.c_void_p(self.pinned.ptr), st)
        if check:
            self.check(rc, "dcvc_frame_analyze")
        self.check(self.lib.dcvc_stream_sync(st), "dcvc_stream_sync")
        return rc, tuple(int(v) for v in self.words)


def _u16_to_numpy(t):
    return t.view(torch.int16).cpu().numpy().view(np.uint16).astype(np.int64)


def _u16_from_numpy(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint16).view(np.int16)).cuda().view(torch.uint16)


def _samples(h, w, np_dtype, seed):
    """values inside and outside [0, 1] with the special ones sprinkled in: 0, 1, the exact tie 0.5 (511.5 -> 512), far
    outside, NaN and infinities, and in fp32 a value whose PRODUCT is the tie 510.5 (-> 510)"""
    rng = np.random.default_rng(seed)
    a = rng.uniform(-0.2, 1.2, (h, w)).astype(np.float32)
    special = [0.0, 1.0, 0.5, -3.0, 7.0, np.nan, np.inf, -np.inf, 0.25, 1.0 / 1023.0]
    if np_dtype == np.float32:
        v = np.float32(510.5 / 1023.0)
        while np.float32(v * np.float32(1023.0)) != np.float32(510.5):
            v = np.nextafter(v, np.float32(2.0), dtype=np.float32)
        special.append(v)
    idx = rng.integers(0, h * w, size=max(len(special), (h * w) // 8))
    a.reshape(-1)[idx] = np.asarray(special, np.float32)[np.arange(idx.size) % len(special)]
    a[0, :8] = 0.5                     # a whole row of ties in block (0, 0)
    return a.astype(np_dtype)


# (h, w, ld, base offset in elements): one block; the smallest plane with all three intra cases; odd block counts; a pitch
# (16-byte accesses); pitches that only allow 8-, 4- and 2-byte accesses of fp16; a misaligned base with an odd pitch
# (single elements); 136 * 240 = 32640 blocks: 510 workgroups of the luma pass, and more blocks than the statistics pass
# has threads (64 workgroups of 256), so its grid-stride loop runs
_CASES = [(8, 8, 8, 0), (16, 16, 16, 0), (24, 40, 40, 0), (136, 200, 208, 0), (136, 200, 204, 0), (136, 200, 202, 0),
          (136, 200, 201, 1), (1088, 1920, 1920, 0)]


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("h,w,ld,off", _CASES)
def test_kernel_equals_the_restatement_bit_for_bit(h, w, ld, off, dtype):
    npd = _NP[dtype]
    luma = _samples(h, w, npd, seed=h * 31 + w + ld)
    host = np.full(off + h * ld + 8, 0.75, npd)                    # (what lies in the pitch is never read as a sample)
    host[off:off + h * ld].reshape(h, ld)[:, :w] = luma
    dev = torch.from_numpy(host).cuda()
    ptr = dev.data_ptr() + off * dev.element_size()
    want_L, want = R.analyze(luma)
    call = _Caller(h, w)
    out = [torch.zeros((h // 8, w // 8), dtype=torch.uint16, device="cuda") for _ in range(3)]
    # without a previous plane
    _, words = call(dtype, ptr, ld, None, out[0])
    assert np.array_equal(_u16_to_numpy(out[0]), want_L)
    assert words == want
    # the same call again: the same words and plane
    _, again = call(dtype, ptr, ld, None, out[1])
    assert again == words and torch.equal(out[0].view(torch.int16), out[1].view(torch.int16))
    # against a previous plane: another frame's, and the extreme values
    prev_L = R.lowres(_samples(h, w, npd, seed=7))
    prev_L.reshape(-1)[::5] = 65472
    prev_L.reshape(-1)[1::7] = 0
    _, words = call(dtype, ptr, ld, _u16_from_numpy(prev_L), out[2])
    assert np.array_equal(_u16_to_numpy(out[2]), want_L)
    assert words == R.analyze(luma, prev_L)[1]
    assert words[0] > 0 and words[1:] == want[1:]


def test_bad_size_is_an_argument_error_and_launches_nothing():
    from opendcvc_amd import _lib
    call = _Caller(12, 16)
    assert _lib.lib().dcvc_frame_analysis_ws_bytes(12, 16) < 0 and _lib.lib().dcvc_frame_analysis_ws_bytes(16, 4) < 0
    assert _lib.lib().dcvc_frame_analysis_ws_bytes(16, 16) > 0
    luma = torch.full((16, 16), 0.5, dtype=torch.float16, device="cuda")
    out = torch.full((2, 2), 7, dtype=torch.int16, device="cuda")
    call.words[:] = 99
    for h, w in ((12, 16), (16, 20), (0, 16), (16, 4)):
        call.h, call.w = h, w
        rc, words = call(torch.float16, luma.data_ptr(), 16, None, out.view(torch.uint16), check=False)
        assert rc < 0 and words == (99, 99, 99, 99), (h, w)
    assert torch.all(out == 7)
    with pytest.raises(_lib.DcvcError, match="multiples of 8"):
        call(torch.float16, luma.data_ptr(), 16, None, out.view(torch.uint16))
    call.h, call.w = 16, 16
    rc, _ = call(torch.float16, luma.data_ptr(), 8, None, out.view(torch.uint16), check=False)      # ld < W
    assert rc < 0 and torch.all(out == 7)
    assert call(torch.float16, luma.data_ptr(), 16, None, out.view(torch.uint16))[1] == (0, 0, 4 * 64 * 512, 4)


# ---------------------------------------------------------------------------------- FrameAnalyzer
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("hw", [(64, 64), (136, 200)])
def test_frame_analyzer_follows_the_sequence(hw, dtype):
    from opendcvc_amd.analysis import FrameAnalyzer, FrameStats, is_cut
    h, w = hw
    an = FrameAnalyzer("cuda:0")
    prev, cuts = None, []
    for fi, f in enumerate(R.two_scene_frames(h, w)):
        if fi == 7:
            an.reset()                       # the previous plane is forgotten: frame 7 is analysed like a first frame
            prev = None
        x = torch.from_numpy(f).to("cuda", dtype)
        got = an.analyze(x)
        L, (inter, intra, total, blocks) = R.analyze(f[0, 0].astype(_NP[dtype]), prev)
        assert got == FrameStats(inter, intra, total, blocks, prev is not None), fi
        if is_cut(got, 150):
            cuts.append(fi)
        prev = L
    assert cuts == [5, 8]
    # an event of the caller's instead of the analyzer's own; a plane with a pitch (a crop of a wider input)
    wide = torch.from_numpy(R.two_scene_frames(h, w + 8, n=1)[0]).to("cuda", dtype)
    ev = torch.cuda.Event()
    ev.record(torch.cuda.current_stream())
    got = an.analyze(wide[:, :, :, 8:], ready=ev)
    assert got[:4] == R.analyze(wide[0, 0, :, 8:].cpu().numpy(), prev)[1] and got.has_prev


# ---------------------------------------------------------------------------------- adaptive I frames, end to end
H = W = 64
QP = 30


def _codecs():
    from opendcvc_amd.models import DMC, DMCI
    i_net, p_net = DMCI(), DMC()
    i_net.load_state_dict({k: torch.from_numpy(v) for k, v in weights.make_state_dict("dmci", 1234).items()})
    p_net.load_state_dict({k: torch.from_numpy(v) for k, v in weights.make_state_dict("dmc", 1234).items()})
    for m in (i_net, p_net):
        m.to("cuda").eval()
        m.update(0.12)
        m.set_use_two_entropy_coders(False)
    return i_net, p_net


@pytest.fixture(scope="module")
def nets():
    """one encoder-side and one decoder-side (DMCI, DMC) pair, fp32, shared by the tests below (models are reusable
    across sequences)"""
    return _codecs() + _codecs()


@pytest.fixture(scope="module")
def two_scenes():
    return [torch.from_numpy(f).cuda() for f in R.two_scene_frames(H, W, n=8)]


@pytest.fixture(scope="module")
def one_scene():
    return [torch.from_numpy(weights.synthetic_frame_yuv444(H, W, i, 3)).cuda() for i in range(8)]


def _container(pkts):
    from opendcvc_amd.bitstream import StreamWriter
    out = io.BytesIO()
    wr = StreamWriter(out)
    for p in pkts:
        wr.write_frame(H, W, False, p)
    return out.getvalue()


def _encode(nets, frames, **kw):
    from opendcvc_amd.pipeline import SequenceEncoder
    enc = SequenceEncoder(nets[0], nets[1], QP, **kw)
    pkts, refs = [], []
    for x in frames:
        r = enc.encode(x)
        pkts += r if kw.get("defer_stream") else [r]
        if not kw.get("defer_stream"):
            ref = nets[1].dpb[0]    # the encoder's own reconstruction: the intra picture, or the P frame's reference feature
            refs.append((ref.frame if ref.feature is None else ref.feature).float().cpu().numpy())
    pkts += enc.flush()
    return enc, pkts, refs


_TYPES = [True, False, False, False, False, True, False, False]        # I P P P P I P P


@pytest.fixture(scope="module")
def sequential(nets, two_scenes):
    """the two-scene material coded with scenecut 150, sent through the container and decoded: (encoder, packets, decoded
    pictures)"""
    from opendcvc_amd.bitstream import StreamReader
    from opendcvc_amd.pipeline import FramePacket, SequenceDecoder
    enc, pkts, refs = _encode(nets, two_scenes, intra_period=-1, reset_interval=3, scenecut=150)
    rd = StreamReader(io.BytesIO(_container(pkts)))
    dec = SequenceDecoder(nets[2], nets[3], H, W, False)
    pics = []
    for fi in range(len(pkts)):
        sps, is_i, qp, payload = rd.read_frame()
        pics.append(dec.decode(FramePacket(is_i, qp, sps["use_ada_i"], payload, chunked=rd.chunked)).float().cpu().numpy())
        ref = nets[3].dpb[0]
        got = (ref.frame if ref.feature is None else ref.feature).float().cpu().numpy()
        assert np.array_equal(got, refs[fi]), f"frame {fi}: decoder and encoder hold different references"
        if is_i:
            assert np.array_equal(pics[-1], refs[fi]), f"frame {fi}: decoded intra picture differs from the encoder's"
    return enc, pkts, pics


def test_cut_starts_a_new_gop_and_the_stream_decodes(nets, sequential):
    enc, pkts, pics = sequential
    assert [p.is_i for p in pkts] == _TYPES and enc.scene_cuts == [5]
    from opendcvc_amd.pipeline import INDEX_MAP
    g = 0
    for fi, p in enumerate(pkts):                              # the P-frame rules count from the cut
        g = 0 if p.is_i else g + 1
        if not p.is_i:
            assert p.qp == nets[1].shift_qp(QP, INDEX_MAP[g % 8]) and p.use_ada_i == int(g % 3 == 1), fi
    assert len(pics) == 8 and all(np.isfinite(x).all() for x in pics)


def test_deferred_stream_gives_the_same_packets(nets, two_scenes, sequential):
    _, want, _ = sequential
    enc, pkts, _ = _encode(nets, two_scenes, intra_period=-1, reset_interval=3, scenecut=150, defer_stream=True)
    assert enc.scene_cuts == [5] and len(pkts) == len(want)
    for fi, (a, b) in enumerate(zip(pkts, want)):
        assert (a.is_i, a.qp, a.use_ada_i, a.bit_stream) == (b.is_i, b.qp, b.use_ada_i, b.bit_stream), fi


def test_two_stage_pipeline_with_a_scenecut_encoder(nets, two_scenes, sequential):
    from opendcvc_amd.pipeline import EncodeDecodePipeline, SequenceDecoder, SequenceEncoder
    _, want, want_pics = sequential
    enc = SequenceEncoder(nets[0], nets[1], QP, intra_period=-1, reset_interval=3, scenecut=150)
    dec = SequenceDecoder(nets[2], nets[3], H, W, False, defer_output=True)
    pkts, pics = [], []
    EncodeDecodePipeline(enc, dec, torch.device("cuda", 0)).run(two_scenes, on_packet=pkts.append,
                                                                on_frame=lambda t: pics.append(t.float().cpu().numpy()))
    assert enc.scene_cuts == [5] and [p.is_i for p in pkts] == _TYPES
    assert [p.bit_stream for p in pkts] == [p.bit_stream for p in want]
    assert len(pics) == 8 and all(np.array_equal(a, b) for a, b in zip(pics, want_pics))


@pytest.mark.parametrize("kw", [dict(intra_period=-1, reset_interval=3), dict(intra_period=32, reset_interval=32)])
def test_without_a_cut_the_container_is_byte_identical(nets, one_scene, kw):
    off, pkts_off, _ = _encode(nets, one_scene, **kw)
    on, pkts_on, _ = _encode(nets, one_scene, scenecut=150, **kw)
    assert on.scene_cuts == [] and off.scene_cuts == [] and off._analyzer is None and on._analyzer is not None
    assert [p.is_i for p in pkts_on] == [True] + [False] * 7
    assert _container(pkts_on) == _container(pkts_off)


def test_harness_reports_the_cut(nets, tmp_path):
    from opendcvc_amd import harness
    src = tmp_path / "two_scenes.yuv"
    with open(src, "wb") as f:
        for i in range(8):
            for plane in weights.synthetic_frame_yuv420(H, W, i, 3 if i < 5 else 11):
                f.write(plane.tobytes())
    kw = dict(intra_period=-1, reset_interval=3, verbose_json=True)
    on = harness.run_one_point(nets[0], nets[1], str(src), W, H, 8, QP, QP, scenecut=150, **kw)
    assert on["frame_type"] == [0, 1, 1, 1, 1, 0, 1, 1] and on["scene_cuts"] == [5]
    assert (on["i_frame_num"], on["p_frame_num"]) == (2, 6)
    off = harness.run_one_point(nets[0], nets[1], str(src), W, H, 8, QP, QP, **kw)
    assert "scene_cuts" not in off and off["frame_type"] == [0] + [1] * 7
    assert list(off) == [k for k in on if k != "scene_cuts"] and list(on)[-1] == "scene_cuts"
    again = harness.run_one_point(nets[0], nets[1], str(src), W, H, 8, QP, QP, scenecut=0, min_keyint=9, **kw)
    assert {k: v for k, v in again.items() if k != "test_time"} == {k: v for k, v in off.items() if k != "test_time"}
