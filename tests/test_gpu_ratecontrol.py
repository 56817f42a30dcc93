"""Target-bitrate control end to end: pipeline.SequenceEncoder(rate=RateController) through the container, the decoder, the
deferred stream, the two-stage pipeline and the harness."""
import io
import math

import numpy as np
import pytest
import torch

from opendcvc_amd import weights

pytestmark = pytest.mark.gpu

H, W = 136, 200


def _codecs(dtype, q_ramp=True):
    from opendcvc_amd.models import DMC, DMCI
    nets = []
    for cls, name in ((DMCI, "dmci"), (DMC, "dmc")):
        m = cls()
        m.load_state_dict({k: torch.from_numpy(v) for k, v in weights.make_state_dict(name, 1234, q_ramp=q_ramp).items()})
        m.to("cuda").eval()
        m.update(0.12)
        if dtype == torch.float16:
            m.half()
        m.set_use_two_entropy_coders(False)
        nets.append(m)
    return nets


@pytest.fixture(scope="module")
def nets():
    """per dtype one encoder-side and one decoder-side (DMCI, DMC) pair with the q_ramp weights"""
    cache = {}

    def get(dtype):
        if dtype not in cache:
            cache[dtype] = _codecs(dtype) + _codecs(dtype)
        return cache[dtype]
    return get


def _frames(dtype, n, seed=3, seed_from=None):
    """padded model inputs of the synthetic clip; seed_from = (frame, seed): another scene from that frame on.  The
    generator's shift wraps every 8 frames, which the scene-cut analysis rightly takes for a cut: the two-scene clip moves
    forth and back instead (frame index 0 .. 7 .. 0), so that its only cut is the change of scene."""
    from opendcvc_amd.pipeline import load_yuv420_frame
    out = []
    for i in range(n):
        s = seed_from[1] if seed_from is not None and i >= seed_from[0] else seed
        k = i if seed_from is None else (i % 14 if i % 14 < 8 else 14 - i % 14)
        y, u, v = (torch.from_numpy(p).cuda() for p in weights.synthetic_frame_yuv420(H, W, k, s))
        out.append(load_yuv420_frame(y, u, v, dtype))
    return out


def _container(pkts):
    from opendcvc_amd.bitstream import StreamWriter
    out = io.BytesIO()
    wr = StreamWriter(out)
    sizes = [wr.write_frame(H, W, False, p) for p in pkts]
    return out.getvalue(), sizes


def _encode(n, frames, qp_i, qp_p=None, keep_refs=False, **kw):
    from opendcvc_amd.pipeline import SequenceEncoder
    for m in n[:2]:
        m.rate_estimate = False
    enc = SequenceEncoder(n[0], n[1], qp_i, qp_p, intra_period=-1, **kw)
    pkts, refs = [], []
    for x in frames:
        r = enc.encode(x)
        pkts += r if kw.get("defer_stream") else [r]
        if keep_refs:
            ref = n[1].dpb[0]
            refs.append((ref.frame if ref.feature is None else ref.feature).float().cpu().numpy())
    pkts += enc.flush()
    return enc, pkts, refs


def _bpp(sizes):
    return 8.0 * sum(sizes) / (len(sizes) * H * W)


def _controller(target_bpp, qp, **kw):
    from opendcvc_amd.ratecontrol import RateController
    return RateController(target_bpp * H * W, qp, **kw)


# ---------------------------------------------------------------------------------- off means off
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_a_pinned_controller_gives_the_fixed_qp_container(nets, dtype):
    n = nets(dtype)
    frames = _frames(dtype, 10)
    off, pkts_off, _ = _encode(n, frames, 36, 30, reset_interval=4)
    want, _ = _container(pkts_off)
    assert off.rate is None and off.rc_qp == [] and not n[0].rate_estimate and not n[1].rate_estimate
    again, pkts_none, _ = _encode(n, frames, 36, 30, reset_interval=4, rate=None)
    assert _container(pkts_none)[0] == want
    for defer in (False, True):
        rc = _controller(0.5, 30, qp_min=30, qp_max=30, qp_i_init=36)
        on, pkts_on, _ = _encode(n, frames, 36, 30, reset_interval=4, rate=rc, defer_stream=defer)
        assert n[0].rate_estimate and n[1].rate_estimate
        got, sizes = _container(pkts_on)
        assert got == want, defer
        assert on.rc_qp == [p.qp for p in pkts_off] and len(on.rc_est_bytes) == len(on.rc_bytes) == 10
        # (an SPS is what write_frame adds on top of a frame's own bytes)
        assert all(0 <= s - b <= 8 for s, b in zip(sizes, on.rc_bytes))
        assert [b for _, b in rc.exact_bytes] == [len(p.bit_stream) for p in pkts_on]


# ---------------------------------------------------------------------------------- the same decisions in every mode
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_modes_take_the_same_decisions(nets, dtype):
    from opendcvc_amd.bitstream import StreamReader
    from opendcvc_amd.pipeline import EncodeDecodePipeline, FramePacket, SequenceDecoder, SequenceEncoder
    n = nets(dtype)
    frames = _frames(dtype, 16)
    target = 0.55
    seq, pkts, refs = _encode(n, frames, 20, rate=_controller(target, 20), keep_refs=True)
    want, _ = _container(pkts)
    assert len(set(seq.rc_qp)) > 3                            # (a real target: the qp moves)
    dfr, pkts_d, _ = _encode(n, frames, 20, rate=_controller(target, 20), defer_stream=True)
    assert dfr.rc_qp == seq.rc_qp and dfr.rc_est_bytes == seq.rc_est_bytes and _container(pkts_d)[0] == want
    assert dfr.rc_bytes == seq.rc_bytes

    # a SequenceDecoder on the container reproduces the encoder's pictures / references
    rd = StreamReader(io.BytesIO(want))
    dec = SequenceDecoder(n[2], n[3], H, W, False)
    pics = []
    for fi in range(len(pkts)):
        sps, is_i, qp, payload = rd.read_frame()
        assert qp == seq.rc_qp[fi]
        pics.append(dec.decode(FramePacket(is_i, qp, sps["use_ada_i"], payload, chunked=rd.chunked)).float().cpu().numpy())
        ref = n[3].dpb[0]
        got = (ref.frame if ref.feature is None else ref.feature).float().cpu().numpy()
        assert np.array_equal(got, refs[fi]), f"frame {fi}: decoder and encoder hold different references"

    for m in n[:2]:
        m.rate_estimate = False
    enc = SequenceEncoder(n[0], n[1], 20, intra_period=-1, rate=_controller(target, 20), defer_stream=True)
    dec = SequenceDecoder(n[2], n[3], H, W, False, defer_output=True)
    pkts_p, pics_p = [], []
    EncodeDecodePipeline(enc, dec, torch.device("cuda", 0)).run(frames, on_packet=pkts_p.append,
                                                                on_frame=lambda t: pics_p.append(t.float().cpu().numpy()))
    assert enc.rc_qp == seq.rc_qp and _container(pkts_p)[0] == want
    assert len(pics_p) == 16 and all(np.array_equal(a, b) for a, b in zip(pics_p, pics))


# ---------------------------------------------------------------------------------- it hits the target
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("cut", [None, 24])
def test_the_target_is_hit(nets, dtype, cut):
    """The clip at fixed qp 32 and 48 (what the parent codes) gives R32 < R48; coded with the target sqrt(R32 * R48) from qp
    16, the last 32 of 48 frames are within one qp step of the measured curve, (R48 / R32) ** (1 / 16) - 1, of the target.
    cut: the scene changes at that frame and --scenecut 150 places an I frame there, inside the measured frames."""
    n = nets(dtype)
    frames = _frames(dtype, 48, seed_from=None if cut is None else (cut, 11))
    kw = dict(scenecut=150) if cut is not None else {}
    rate = {}
    for qp in (32, 48):
        enc, pkts, _ = _encode(n, frames, qp, **kw)
        assert enc.scene_cuts == ([] if cut is None else [cut])
        rate[qp] = _bpp(_container(pkts)[1])
    assert rate[32] < rate[48]
    target = math.sqrt(rate[32] * rate[48])
    step = (rate[48] / rate[32]) ** (1.0 / 16.0) - 1.0
    enc, pkts, _ = _encode(n, frames, 16, rate=_controller(target, 16), **kw)
    sizes = _container(pkts)[1]
    got = _bpp(sizes[16:])
    print(f"{dtype} cut {cut}: R32 {rate[32]:.4f} R48 {rate[48]:.4f} target {target:.4f} bpp, last 32 frames {got:.4f} "
          f"({got / target - 1:+.4f}, one step {step:.4f}), all 48 {_bpp(sizes):.4f}, qp {enc.rc_qp}")
    assert enc.scene_cuts == ([] if cut is None else [cut]) and [p.is_i for p in pkts].count(True) == (1 if cut is None else 2)
    assert all(0 <= p.qp <= 63 + 8 for p in pkts) and all(0 <= q <= 71 for q in enc.rc_qp)
    assert pkts[0].qp == 16
    assert abs(got / target - 1.0) <= step


# ---------------------------------------------------------------------------------- the harness
def test_harness_logs_the_rate_control_keys(nets, tmp_path):
    from opendcvc_amd import harness
    n = nets(torch.float16)
    src = tmp_path / "clip.yuv"
    with open(src, "wb") as f:
        for i in range(12):
            for plane in weights.synthetic_frame_yuv420(H, W, i, 3):
                f.write(plane.tobytes())
    kw = dict(intra_period=-1, reset_interval=32, verbose_json=True)
    off = harness.run_one_point(n[0], n[1], str(src), W, H, 12, 32, 32, **kw)
    on = harness.run_one_point(n[0], n[1], str(src), W, H, 12, 32, 32, target_bpp=0.5, **kw)
    new = ["target_bpp", "rc_qp", "rc_est_bpp", "frame_rc_qp", "frame_rc_est_bpp"]
    assert list(on) == list(off) + new and not set(new) & set(off)
    assert on["target_bpp"] == 0.5 and len(on["frame_rc_qp"]) == len(on["frame_rc_est_bpp"]) == 12
    assert abs(on["rc_est_bpp"] / on["ave_all_frame_bpp"] - 1.0) <= 0.01
    assert abs(on["rc_qp"] - np.mean(on["frame_rc_qp"])) < 1e-9 and len(set(on["frame_rc_qp"])) > 2
    brief = harness.run_one_point(n[0], n[1], str(src), W, H, 12, 32, 32, target_bpp=0.5, intra_period=-1)
    assert list(brief)[-3:] == new[:3] and "frame_rc_qp" not in brief
    again = harness.run_one_point(n[0], n[1], str(src), W, H, 12, 32, 32, **kw)
    assert again["frame_bpp"] == off["frame_bpp"] and not n[0].rate_estimate and not n[1].rate_estimate
