"""Decoder-state digests on the GPU: dcvc_state_digest against the numpy restatement bit for bit, and the digests end to end
through pipeline.SequenceEncoder(digest=True), the container, SequenceDecoder, the two-stage pipeline and the harness."""
import io
import json
import os

import numpy as np
import pytest
import torch

from digest_ref import digest_ref, strip_digest_units
from opendcvc_amd import _lib, weights

pytestmark = pytest.mark.gpu

PASS = _lib.DIGEST_PASS_WORDS                   # words one grid-stride pass of the kernel's full grid covers
WORDS = [1, 2, 255, 256, 257, 12345, PASS - 1, PASS, PASS + 1, 3 * PASS + 5]
N_FRAMES, INTRA = 6, 4                          # I P P P I P


# ---------------------------------------------------------------------------------- the kernel
@pytest.fixture(scope="module")
def blob():
    """random bytes for the largest case plus one word, on both sides, and the reference digests - computed once per
    (offset, words), shared, never modified"""
    host = np.random.default_rng(7).integers(0, 256, 8 * (max(WORDS) + 1), dtype=np.uint8)
    dev = torch.from_numpy(host).cuda()
    assert dev.data_ptr() % 16 == 0
    cache = {}

    def ref(first_word, m):
        if (first_word, m) not in cache:
            cache[(first_word, m)] = digest_ref(host[8 * first_word:8 * (first_word + m)].tobytes())
        return cache[(first_word, m)]
    return dev, ref


@pytest.fixture(scope="module")
def digester():
    from opendcvc_amd.digest import StateDigest
    return StateDigest("cuda:0")


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("m", WORDS)
def test_kernel_equals_the_restatement(blob, digester, m, dtype):
    dev, ref = blob
    x = dev[:8 * m].view(dtype)
    assert x.is_contiguous() and x.numel() * x.element_size() == 8 * m
    h = digester.enqueue(x)
    want = ref(0, m)
    print(f"{m} words as {dtype}: {h.value():#018x} against {want:#018x}")
    assert h.value() == want and h.status() == 0


@pytest.mark.parametrize("m", [1, 2, 256, 257, 12345, PASS, PASS + 1])
def test_view_that_starts_8_bytes_into_an_aligned_allocation(blob, digester, m):
    dev, ref = blob
    x = dev[8:8 + 8 * m].view(torch.float16)
    assert x.data_ptr() % 16 == 8
    assert digester.enqueue(x).value() == ref(1, m)


def test_status_word(blob, digester):
    dev, ref = blob
    for m in (1, 257, PASS + 1):
        x, want = dev[:8 * m].view(torch.float32), ref(0, m)
        handles = [digester.enqueue(x, e) for e in (want, want ^ 1, want ^ (1 << 63), 0, 2 ** 64 - 1)] + [digester.enqueue(x)]
        assert [h.status() for h in handles] == [1, 2, 2, 2, 2, 0]
        assert all(h.value() == want for h in handles)


def test_handles_outlive_their_ring_slot(blob, digester):
    from opendcvc_amd.digest import RING
    dev, ref = blob
    sizes = [1 + k for k in range(2 * RING + 3)]
    handles = [digester.enqueue(dev[:8 * m].view(torch.float16)) for m in sizes]       # none read before the ring came round
    assert [h.value() for h in handles] == [ref(0, m) for m in sizes]
    with pytest.raises(AssertionError):
        digester.enqueue(dev[:64].view(torch.float16)[::2])


# ---------------------------------------------------------------------------------- sequences
def _codecs(rec, dtype):
    from opendcvc_amd.models import DMC, DMCI
    nets = []
    for cls, name in ((DMCI, "dmci"), (DMC, "dmc")):
        m = cls()
        m.load_state_dict({k: torch.from_numpy(v) for k, v in weights.make_state_dict(name, rec["seed"]).items()})
        m.to("cuda").eval()
        m.update(rec["thres"])
        if dtype == torch.float16:
            m.half()
        m.set_use_two_entropy_coders(bool(rec["two"]))
        nets.append(m)
    return nets


@pytest.fixture(scope="module")
def world(golden_dir):
    """per (record, dtype): the record, an encoder-side and a decoder-side (DMCI, DMC) pair, the frames"""
    recs = json.load(open(os.path.join(golden_dir, "sequences.json")))
    cache = {}

    def get(name, dtype):
        if (name, dtype) not in cache:
            rec = recs[name]
            assert (rec["h"], rec["w"]) == (64, 64)
            frames = [torch.from_numpy(weights.synthetic_frame_yuv444(64, 64, fi, 0)).to("cuda", dtype) for fi in range(N_FRAMES)]
            cache[(name, dtype)] = (rec, _codecs(rec, dtype) + _codecs(rec, dtype), frames)
        return cache[(name, dtype)]
    yield get
    cache.clear()


def _mode(nets, entropy):
    for m in nets:
        m.entropy = entropy
        m.rate_estimate = False


def _entry_bytes(p_net):
    ref = p_net.dpb[0]
    t = ref.frame if ref.feature is None else ref.feature
    return t.contiguous().view(torch.uint8).cpu().numpy().tobytes()


def _encode(w, defer=False, entries=None, **kw):
    from opendcvc_amd.pipeline import SequenceEncoder
    rec, nets, frames = w
    enc = SequenceEncoder(nets[0], nets[1], rec["qp"], intra_period=INTRA, reset_interval=rec["reset_interval"],
                          defer_stream=defer, **kw)
    pkts = []
    for x in frames:
        r = enc.encode(x)
        pkts += r if defer else [r]
        if entries is not None:
            entries.append(_entry_bytes(nets[1]))
    pkts += enc.flush()
    return enc, pkts


def _container(w, pkts):
    from opendcvc_amd.bitstream import StreamWriter
    out = io.BytesIO()
    wr = StreamWriter(out)
    sizes = [wr.write_frame(w[0]["h"], w[0]["w"], bool(w[0]["two"]), p) for p in pkts]
    return out.getvalue(), sizes


def _read(data, n):
    from opendcvc_amd.bitstream import StreamReader
    from opendcvc_amd.pipeline import FramePacket
    rd = StreamReader(io.BytesIO(data))
    out = []
    for _ in range(n):
        sps, is_i, qp, payload = rd.read_frame()
        out.append(FramePacket(is_i, qp, sps["use_ada_i"], payload, chunked=rd.chunked, digest=rd.digest))
    return out


def _decoder(w, defer=False):
    from opendcvc_amd.pipeline import SequenceDecoder
    rec, nets, _ = w
    return SequenceDecoder(nets[2], nets[3], rec["h"], rec["w"], bool(rec["two"]), defer_output=defer)


def _decode(w, pkts, defer=False):
    dec = _decoder(w, defer)
    pics = []
    for p in pkts:
        r = dec.decode(p)
        pics += r if defer else [r]
    pics += dec.flush()
    return dec, [t.float().cpu().numpy() for t in pics]


@pytest.mark.parametrize("entropy", ["host", "device"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("name", ["seq_64", "seq_64_two"])
def test_every_frame_is_checked_in_every_mode(world, name, dtype, entropy):
    from opendcvc_amd.pipeline import EncodeDecodePipeline
    w = world(name, dtype)
    _mode(w[1], entropy)
    off_enc, off = _encode(w)
    assert not off_enc.digest and off_enc._digester is None and all(p.digest is None for p in off)     # off: nothing launched
    assert [p.is_i for p in off] == [True, False, False, False, True, False]
    assert all(p.chunked == (entropy == "device") for p in off)
    want, _ = _container(w, off)
    off_dec, pics = _decode(w, off)
    assert off_dec.digests_checked == 0 and off_dec._digester is None and len(pics) == N_FRAMES

    entries, digests = [], None
    for defer in (False, True):
        _, pkts = _encode(w, defer, entries=entries if not defer else None, digest=True)
        assert [p.bit_stream for p in pkts] == [p.bit_stream for p in off], defer
        assert [(p.is_i, p.qp, p.use_ada_i, p.chunked) for p in pkts] == [(p.is_i, p.qp, p.use_ada_i, p.chunked) for p in off]
        if digests is None:
            digests = [p.digest for p in pkts]
            # what the stream carries is the digest, as defined, of the entry the frame put into the encoder's DPB
            assert digests == [digest_ref(e) for e in entries]
            assert len(set(digests)) == N_FRAMES
        assert [p.digest for p in pkts] == digests, defer
        data, sizes = _container(w, pkts)
        stripped, units = strip_digest_units(data, pkts, sizes)
        assert stripped == want and units == digests
        back = _read(data, N_FRAMES)
        assert back == pkts
        for defer_out in (False, True):
            dec, got = _decode(w, back, defer_out)
            assert dec.digests_checked == N_FRAMES, (defer, defer_out)
            assert len(got) == N_FRAMES and all(np.array_equal(a, b) for a, b in zip(got, pics))
        # the two-stage pipeline: packets handed over as objects
        from opendcvc_amd.pipeline import SequenceEncoder
        rec, nets, frames = w
        enc = SequenceEncoder(nets[0], nets[1], rec["qp"], intra_period=INTRA, reset_interval=rec["reset_interval"],
                              defer_stream=defer, digest=True)
        dec = _decoder(w, defer)
        piped, got = [], []
        EncodeDecodePipeline(enc, dec, torch.device("cuda", 0)).run(frames, on_packet=piped.append,
                                                                    on_frame=lambda t: got.append(t.float().cpu().numpy()))
        assert piped == pkts and dec.digests_checked == N_FRAMES, defer
        assert len(got) == N_FRAMES and all(np.array_equal(a, b) for a, b in zip(got, pics))


def _move_one_ulp(feature):
    """the element of largest magnitude (a normal number: the next bit pattern is the next value) moved by one ulp, in place"""
    f16 = feature.dtype == torch.float16
    bits = feature.view(torch.int16 if f16 else torch.int32).view(-1)
    at = int(feature.float().abs().view(-1).argmax())
    before = float(feature.view(-1)[at])
    bits[at] += 1
    after = float(feature.view(-1)[at])
    assert after != before and abs(after - before) <= abs(before) * 2.0 ** (-10 if f16 else -23)


def test_drift_is_caught_at_the_frame_where_it_starts(world):
    """one element of the decoder's reference feature moved by one ulp behind frame 2: frame 2 has passed, frame 3 - decoded
    from the moved feature - is the first whose entry differs.  An ordinary comparison of two values: no device fault.
    fp32, where a step of 2^-23 is far too small to move a symbol into another cdf table: the stream decodes, the pictures
    are (slightly) wrong, and only the digest says so.  (Measured at the magnitude quantiles 0.01 .. 1 of the feature's
    elements: frame 3's entry then differs in about 16.5 K of its 65.5 K bytes.)"""
    w = world("seq_64", torch.float32)
    _mode(w[1], "host")
    _, pkts = _encode(w, digest=True)
    p_dec = w[1][3]
    for defer in (False, True):
        dec = _decoder(w, defer)
        for p in pkts[:3]:
            dec.decode(p)
        assert p_dec.dpb[0].feature is not None and p_dec.dpb[0].feature.dtype == torch.float32
        _move_one_ulp(p_dec.dpb[0].feature)
        with pytest.raises(_lib.DigestMismatch) as e:
            dec.decode(pkts[3])
            dec.flush()
        assert e.value.index == 3 and not e.value.is_i and e.value.expected == pkts[3].digest and e.value.got != pkts[3].digest
        assert dec.digests_checked == 3, defer
        assert "frame 3" in str(e.value) and f"{pkts[3].digest:#018x}" in str(e.value) and f"{e.value.got:#018x}" in str(e.value)
        p_dec.finish_output()                                      # (leave no deferred picture behind for the next decoder)
    torch.cuda.synchronize()                                       # (the device is well: nothing faulted)


def test_fp16_drift_never_passes_silently(world):
    """The same step in fp16 is 2^-10 of the element: it moves a scale index across a threshold of the cdf tables, the
    symbols are mis-decoded and the entropy coder's end-state check refuses frame 3 before it enters the DPB - the other
    detector, a plain DcvcError for the same frame (measured at the magnitude quantiles 0.1 .. 1 of the feature's elements;
    the step of an element of magnitude 1.6e-3 or less rounds away before it reaches frame 3's entry, which then equals the
    encoder's: there is no drift to report).  Either way frame 3 does not pass, and frames 0 .. 2 have."""
    w = world("seq_64", torch.float16)
    _mode(w[1], "host")
    _, pkts = _encode(w, digest=True)
    p_dec = w[1][3]
    dec = _decoder(w)
    for p in pkts[:3]:
        dec.decode(p)
    _move_one_ulp(p_dec.dpb[0].feature)
    with pytest.raises(_lib.DcvcError) as e:
        dec.decode(pkts[3])
        dec.flush()
    print(f"fp16: frame 3 refused by {type(e.value).__name__}: {e.value}")
    assert not isinstance(e.value, _lib.DigestMismatch) or e.value.index == 3
    assert dec.digests_checked == 3
    torch.cuda.synchronize()


@pytest.mark.parametrize("frame", [2, 4])
def test_a_flipped_bit_in_a_digest_unit_is_reported_for_its_frame(world, frame):
    w = world("seq_64", torch.float16)
    _mode(w[1], "host")
    _, pkts = _encode(w, digest=True)
    data, sizes = _container(w, pkts)
    from opendcvc_amd.bitstream import frame_overhead_bytes
    n = len(pkts[frame].bit_stream)
    at = sum(sizes[:frame + 1]) - n - frame_overhead_bytes(n) - 9            # the unit stands in front of the frame unit
    assert data[at] >> 4 == 5
    bad = bytearray(data)
    bad[at + 1 + 5] ^= 0x08
    back = _read(bytes(bad), N_FRAMES)
    assert back[frame].digest == pkts[frame].digest ^ (0x08 << 40)
    dec = _decoder(w)
    with pytest.raises(_lib.DigestMismatch) as e:
        for p in back[:frame + 1]:
            dec.decode(p)
        dec.check_digests()
    assert e.value.index == frame and e.value.is_i == (frame == 4)
    assert e.value.expected == back[frame].digest and e.value.got == pkts[frame].digest
    assert dec.digests_checked == frame


def test_digests_compose_with_scenecut_and_rate_control(world):
    """a controller held at one qp codes the packets of the fixed qp; the digest unit's 9 bytes are in what it is fed and in
    rc_bytes, frame by frame"""
    from opendcvc_amd.ratecontrol import RateController
    w = world("seq_64", torch.float16)
    rec, nets, _ = w
    _mode(nets, "host")
    runs = {}
    try:
        for digest in (False, True):
            rc = RateController(0.5 * 64 * 64, rec["qp"], qp_min=rec["qp"], qp_max=rec["qp"], qp_i_init=rec["qp"])
            runs[digest] = _encode(w, scenecut=150, rate=rc, digest=digest)
    finally:
        _mode(nets, "host")
    (enc_off, off), (enc_on, on) = runs[False], runs[True]
    assert [p.bit_stream for p in on] == [p.bit_stream for p in off] and enc_on.scene_cuts == enc_off.scene_cuts
    assert enc_on.rc_qp == enc_off.rc_qp and len(enc_on.rc_bytes) == N_FRAMES
    assert [a - b for a, b in zip(enc_on.rc_bytes, enc_off.rc_bytes)] == [9] * N_FRAMES
    assert [a - b for a, b in zip(enc_on.rc_est_bytes, enc_off.rc_est_bytes)] == [9] * N_FRAMES
    _, sizes = _container(w, on)
    assert all(0 <= s - b <= 8 for s, b in zip(sizes, enc_on.rc_bytes))          # (an SPS is all write_frame adds on top)
    assert all(p.digest is not None for p in on) and all(p.digest is None for p in off)
    dec, _ = _decode(w, on, defer=True)
    assert dec.digests_checked == N_FRAMES


def test_harness_checks_every_frame(world, tmp_path):
    from opendcvc_amd import harness
    H, W, N = 136, 200, 6
    _, nets, _ = world("seq_64", torch.float16)
    _mode(nets, "host")
    src = tmp_path / "clip.yuv"
    with open(src, "wb") as f:
        for i in range(N):
            for plane in weights.synthetic_frame_yuv420(H, W, i, 3):
                f.write(plane.tobytes())
    kw = dict(intra_period=INTRA, reset_interval=32, verbose_json=True)
    off = harness.run_one_point(nets[0], nets[1], str(src), W, H, N, 32, 32, bin_path=str(tmp_path / "off.bin"), **kw)
    on = harness.run_one_point(nets[0], nets[1], str(src), W, H, N, 32, 32, bin_path=str(tmp_path / "on.bin"), digest=True, **kw)
    assert list(on) == list(off) + ["digests_checked"] and on["digests_checked"] == N
    for k in off:
        if k == "test_time":
            continue
        if k.endswith("bpp"):                   # 9 bytes per frame more, nothing else
            a, b = np.asarray(on[k], np.float64), np.asarray(off[k], np.float64)
            assert np.allclose(a - b, 72.0 / (H * W), rtol=0, atol=1e-12), k
        else:
            assert on[k] == off[k], k
    assert os.path.getsize(tmp_path / "on.bin") == os.path.getsize(tmp_path / "off.bin") + 9 * N
    for m in nets[:2]:
        m.set_use_two_entropy_coders(False)
