"""Film grain on the host (docs/film_grain.md): the numpy restatement tests/grain_ref.py against the doc's figures, the
estimator closed over the restatement's own synthesis, grain.params_from_stats, the container's grain unit and the options'
way through the encoder and the command line.  No GPU."""
import hashlib
import io
import json
import math
import os

import numpy as np
import pytest

import grain_ref as G
from opendcvc_amd import bitstream as B
from opendcvc_amd import grain
from opendcvc_amd.grain import GrainParams, params_from_stats
from opendcvc_amd.pipeline import FramePacket, SequenceEncoder

N_SIDE = 256
EXCESS_KURTOSIS_WHITE = -1.2 * (256 ** 2 + 1) / (256 ** 2 - 1) / 4        # a sum of four independent uniform bytes


def _autocorr2(corr):
    """sum over all 2-D lags of the shape's squared autocorrelation: N / this is the effective sample count of a variance"""
    t = np.asarray(G.TAPS[corr], np.float64)
    ac = np.correlate(t, t, "full") / (t * t).sum()
    return float((ac * ac).sum()) ** 2


# ---------------------------------------------------------------------------------- the fields
def test_white_field_moments_and_keys():
    n = G.white(1234, 0, 0, 0, 0, N_SIDE, N_SIDE).astype(np.float64)
    N = n.size
    assert n.min() >= -510 and n.max() <= 510 and G.VAR_WHITE == 4 * (256 ** 2 - 1) // 12
    se_mean = math.sqrt(G.VAR_WHITE / N)
    se_var = G.VAR_WHITE * math.sqrt((2 + EXCESS_KURTOSIS_WHITE) / N)
    print("white: mean", n.mean(), "+-", se_mean, "var", n.var(), "+-", se_var)
    assert abs(n.mean()) <= 4 * se_mean
    assert abs((n * n).mean() - G.VAR_WHITE) <= 4 * se_var
    # lag-1 correlation of the white field is 0 within 4 / sqrt(N)
    for a, b in ((n[:, :-1], n[:, 1:]), (n[:-1], n[1:])):
        assert abs((a * b).mean() / G.VAR_WHITE) <= 4 / math.sqrt(a.size)
    base = G.white(1234, 0, 0, 0, 0, 64, 64)
    for other in (G.white(1235, 0, 0, 0, 0, 64, 64), G.white(1234, 1, 0, 0, 0, 64, 64), G.white(1234, 0, 1, 0, 0, 64, 64),
                  G.white(1234, 0, 2, 0, 0, 64, 64), G.white(1234, 5, 0, 0, 0, 64, 64)):
        r = float((base * other).mean()) / G.VAR_WHITE
        assert not np.array_equal(base, other) and abs(r) <= 4 / 64
    # defined two samples beyond the edge, and a window of the field is the field
    assert np.array_equal(G.white(7, 3, 1, -2, -2, 20, 20)[2:, 2:], G.white(7, 3, 1, 0, 0, 18, 18))


@pytest.mark.parametrize("corr", [0, 1, 2])
def test_shaped_field_variance_and_lag1(corr):
    taps2 = sum(a * a for a in G.TAPS[corr]) ** 2
    assert taps2 == (1, 36, 4900)[corr]
    var = G.VAR_WHITE * taps2
    assert var == (21845, 786420, 107040500)[corr]
    assert G.GAIN[corr] == round(2 ** 19 / math.sqrt(var)) == grain.GAIN[corr]
    assert 510 * sum(G.TAPS[corr]) ** 2 * G.GAIN[corr] * 255 < 2 ** 31           # the product is an int32
    g = G.shaped(99, corr, 0, 0, N_SIDE, N_SIDE).astype(np.float64)
    n_eff = g.size / _autocorr2(corr)
    se_var = var * math.sqrt(2 / n_eff)                 # (Gaussian bound: the white field's own kurtosis is below it)
    print(f"corr {corr}: var {(g * g).mean():.1f} expected {var} +- {se_var:.1f} (n_eff {n_eff:.0f})")
    assert abs(g.mean()) <= 4 * math.sqrt(var / n_eff) * 2
    assert abs((g * g).mean() - var) <= 4 * se_var
    lag = 0.5 * ((g[:, :-1] * g[:, 1:]).mean() + (g[:-1] * g[1:]).mean()) / var
    assert abs(lag - grain.LAG1[corr]) <= 4 / math.sqrt(n_eff)
    assert grain.LAG1 == (0.0, 4 / 6, 56 / 70)
    assert grain.CORR_THRESHOLDS == pytest.approx((1 / 3, 11 / 15))
    assert grain.GAIN_RATIO[corr] == pytest.approx((0.99992470, 0.99964279, 1.00640856)[corr], abs=1e-8)
    assert grain.BLOCK_MEAN_SHARE[corr] == pytest.approx((1 / 256, 0.025235, 0.045346)[corr], abs=1e-6)


# ---------------------------------------------------------------------------------- application
def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint16 if a.dtype == np.float16 else np.uint32)


@pytest.mark.parametrize("ndt", [np.float32, np.float16])
def test_zero_strength_is_the_identity_bit_for_bit(ndt):
    rng = np.random.default_rng(3)
    x = (rng.random((3, 32, 48), dtype=np.float32) * 3 - 1).astype(ndt)
    x[0, 0, :4] = [-0.0, 0.0, np.nan, np.inf]
    out = G.apply(x, (20, 40), 5, 2, (0,) * 8, 0, 0, 3)
    assert np.array_equal(_bits(out), _bits(x))
    # luma off, chroma on: luma and everything outside the picture keep their bits, chroma moves
    out = G.apply(x, (20, 40), 5, 1, (0,) * 8, 40, 0, 3)
    assert np.array_equal(_bits(out[0]), _bits(x[0])) and np.array_equal(_bits(out[2]), _bits(x[2]))
    assert np.array_equal(_bits(out[1, 20:]), _bits(x[1, 20:])) and np.array_equal(_bits(out[1, :, 40:]), _bits(x[1, :, 40:]))
    assert (_bits(out[1, :20, :40]) != _bits(x[1, :20, :40])).mean() > 0.9


def test_values_outside_0_1_pass_unclamped_and_the_add_is_the_docs():
    x = np.empty((3, 16, 32), np.float32)
    x[0], x[1], x[2] = 1.5, -0.25, 0.5
    sy = (10, 20, 30, 40, 50, 60, 70, 200)
    out = G.apply(x, (16, 32), 77, 0, sy, 100, 150, 2)
    for c, s in ((0, 200), (1, 100), (2, 150)):          # luma above 1 takes the last band's strength
        p = (G.white(77, 2, c, 0, 0, 16, 32).astype(np.int64) * G.GAIN[0] * s).astype(np.int32)
        want = (x[c] + p.astype(np.float32) * np.float32(2.0 ** -30)).astype(np.float32)
        assert np.array_equal(_bits(out[c]), _bits(np.where(p == 0, x[c], want)))
    assert out[0].max() > 1.5 and out[1].min() < -0.25          # nothing was clamped
    # the added standard deviation is s * 2^-11 * r (4 standard errors of 512 samples' standard deviation)
    sd = float((out[2] - x[2]).std())
    assert abs(sd / (150 * 2.0 ** -11 * grain.GAIN_RATIO[0]) - 1) <= 4 / math.sqrt(2 * 512)


def test_luma_strength_lerp_and_its_end_points():
    sy = (8, 40, 72, 104, 136, 168, 200, 255)
    q = np.arange(256)
    v = (q / 255.0).astype(np.float32)
    assert np.array_equal(np.rint(v * np.float32(255)).astype(int), q)
    s = G.luma_strength(v, sy)
    assert np.all(s[:17] == 8) and np.all(s[240:] == 255)
    for k in range(8):
        assert s[16 + 32 * k] == sy[k]                     # the band centres
    for k in range(7):
        assert s[32 + 32 * k] == (sy[k] + sy[k + 1] + 1) >> 1          # halfway
        assert np.all(np.diff(s[16 + 32 * k:49 + 32 * k]) >= 0)
    assert G.luma_strength(np.asarray([-3.0, 7.0, np.nan], np.float32), sy).tolist() == [8, 255, 8]


# ---------------------------------------------------------------------------------- the estimator on the restatement
TRUE_Y = (24, 32, 40, 48, 56, 64, 72, 80)


@pytest.fixture(scope="module")
def picture():
    x = G.estimator_picture()
    x.setflags(write=False)
    return x


def test_the_picture_gives_every_band_sixteen_flat_blocks(picture):
    assert picture.shape == (3, 144, 256)
    table = G.stats(picture, picture, (144, 256))
    assert table[:8, 0].tolist() == [16] * 8 and table[8:, 0].tolist() == [128] * 4          # no checker-strip block counted
    assert not table[:, 1].any()
    cq = np.rint(picture[0] * 4096)
    assert (256 * (cq[128:, :16] ** 2).sum() - cq[128:, :16].sum() ** 2) > G.FLAT_T


@pytest.mark.parametrize("corr", [0, 1, 2])
def test_estimator_recovers_what_the_restatement_synthesised(picture, corr):
    noisy = G.apply(picture, (144, 256), 4321, corr, TRUE_Y, 36, 52, 0)
    table = G.stats(noisy, picture, (144, 256))
    assert table[:8, 0].tolist() == [16] * 8 and table[8:, 0].tolist() == [128] * 4
    p = params_from_stats(table, 9)
    assert p is not None and p.seed == 9 and p.corr == corr
    # the strength actually applied in a band: the lerp at the step's own 8-bit value
    truth = [int(G.luma_strength(picture[0, 0, 32 * k:32 * k + 1], TRUE_Y)[0]) for k in range(8)]
    rel = lambda blocks: 4 / math.sqrt(2 * blocks * 256 / _autocorr2(corr))
    print(f"corr {corr}: truth {truth} got {p.scale_y} (bound {rel(16):.4f} relative + 0.5), cb {p.scale_cb} cr {p.scale_cr}")
    for k in range(8):
        assert abs(p.scale_y[k] - truth[k]) <= rel(16) * truth[k] + 0.5
    assert abs(p.scale_cb - 36) <= rel(128) * 36 + 0.5 and abs(p.scale_cr - 52) <= rel(128) * 52 + 0.5


# ---------------------------------------------------------------------------------- params_from_stats
def _line(count, strength, corr=0):
    var = (2 * strength * grain.GAIN_RATIO[corr]) ** 2 * (1 - grain.BLOCK_MEAN_SHARE[corr])
    return [count, int(round(count * 65536 * var))]


def test_params_from_stats_empty_single_band_and_zero():
    empty = np.zeros((12, 2), np.int64)
    assert params_from_stats(empty, 1) is None
    t = empty.copy()
    t[3] = _line(grain.MIN_BLOCKS, 50)
    t[2] = _line(grain.MIN_BLOCKS - 1, 200)               # too few blocks: not populated
    t[8] = _line(grain.MIN_BLOCKS, 20)
    p = params_from_stats(t, 0x12345)
    assert p == GrainParams(0x2345, 0, (50,) * 8, 20, 0)
    t[6] = _line(10, 90)
    assert params_from_stats(t, 0).scale_y == (50, 50, 50, 50, 50, 90, 90, 90)        # a tie goes to the lower band
    weak = empty.copy()
    weak[0] = _line(100, 0.4)
    weak[9] = _line(100, 0.3)
    assert params_from_stats(weak, 0) is None
    weak[0] = _line(100, 0.6)
    assert params_from_stats(weak, 0).scale_y == (1,) * 8
    strong = empty.copy()
    strong[0] = [4, 4 * 65536 * 2047 ** 2]
    assert params_from_stats(strong, 0).scale_y == (255,) * 8
    # corr from the lag lines
    for corr in (0, 1, 2):
        t = empty.copy()
        t[4] = _line(50, 60, corr)
        t[10] = t[11] = [50, int(240 * t[4][1] * grain.LAG1[corr])]
        assert params_from_stats(t, 0) == GrainParams(0, corr, (60,) * 8, 0, 0)
    with pytest.raises(ValueError):
        params_from_stats(empty[:11], 0)


def test_grain_params_validate():
    p = GrainParams(65535, 2, range(8), 255, 0)
    assert p.scale_y == tuple(range(8)) and p.active and not GrainParams().active
    assert len(p.to_bytes()) == 13 and GrainParams.from_bytes(p.to_bytes()) == p
    assert p.to_bytes() == bytes([255, 255, 2, 0, 1, 2, 3, 4, 5, 6, 7, 255, 0])
    for bad in (dict(seed=65536), dict(seed=-1), dict(corr=3), dict(scale_y=(0,) * 7), dict(scale_y=(256,) + (0,) * 7),
                dict(scale_cb=-1), dict(scale_cr=256)):
        with pytest.raises(ValueError):
            GrainParams(**bad)
    with pytest.raises(ValueError):
        GrainParams.from_bytes(bytes(12))


# ---------------------------------------------------------------------------------- the container
P1 = GrainParams(513, 1, (1, 2, 3, 4, 5, 6, 7, 8), 9, 10)
P2 = GrainParams(7, 2, (30,) * 8, 0, 0)


def _stream(pkts):
    f = io.BytesIO()
    w = B.StreamWriter(f)
    sizes = [w.write_frame(64, 96, False, p) for p in pkts]
    return f.getvalue(), sizes


def test_grain_unit_round_trip_order_and_counter():
    assert B.NalType.NAL_GRAIN == 7 and B.GRAIN_UNIT_BYTES == 14
    f = io.BytesIO()
    assert B.write_grain(f, 3, P1) == 14 and f.getvalue()[0] == (7 << 4) | 3 and f.getvalue()[1:] == P1.to_bytes()
    r = io.BytesIO(f.getvalue())
    assert B.read_header(r) == {"nal_type": B.NalType.NAL_GRAIN, "sps_id": 3} and B.read_grain_remaining(r) == P1
    assert FramePacket(True, 1, 0, b"x").grain is None
    pay = lambda k: bytes([k]) * (10 + k)
    pkts = [FramePacket(True, 20, 0, pay(0), grain=P1, digest=11), FramePacket(False, 21, 0, pay(1), digest=12),
            FramePacket(False, 22, 0, pay(2)), FramePacket(True, 20, 0, pay(3), grain=P2), FramePacket(False, 21, 0, pay(4)),
            FramePacket(True, 20, 0, pay(5), grain=GrainParams(seed=1)), FramePacket(False, 21, 0, pay(6)),
            FramePacket(True, 20, 0, pay(7))]
    data, sizes = _stream(pkts)
    plain, plain_sizes = _stream([FramePacket(p.is_i, p.qp, p.use_ada_i, p.bit_stream, digest=p.digest) for p in pkts])
    assert sum(sizes) == len(data) == len(plain) + 3 * 14
    assert [a - b for a, b in zip(sizes, plain_sizes)] == [14, 0, 0, 14, 0, 14, 0, 0]
    # SPS, grain, digest, frame
    assert data[4] >> 4 == 7 and data[18] >> 4 == 5 and data[27] >> 4 == 1
    rd = B.StreamReader(io.BytesIO(data))
    assert rd.grain is None
    seen = []
    for p in pkts:
        sps, is_i, qp, payload = rd.read_frame()
        assert (is_i, qp, payload, rd.digest) == (p.is_i, p.qp, p.bit_stream, p.digest)
        seen.append((rd.grain, rd.grain_t))
    # an all-zero unit switches grain off; an I frame without a unit changes nothing
    assert seen == [(P1, 0), (P1, 1), (P1, 2), (P2, 0), (P2, 1), (None, 0), (None, 1), (None, 2)]
    rd = B.StreamReader(io.BytesIO(plain))
    for _ in pkts:
        rd.read_frame()
        assert rd.grain is None


def test_grain_unit_errors():
    data, _ = _stream([FramePacket(True, 20, 0, b"abc", grain=P1, digest=5)])
    sps, grain_unit, digest_unit, frame = data[:4], data[4:18], data[18:27], data[27:]
    B.StreamReader(io.BytesIO(sps + grain_unit + digest_unit + frame)).read_frame()
    with pytest.raises(ValueError, match="digest unit is followed by NAL_GRAIN"):
        B.StreamReader(io.BytesIO(sps + digest_unit + grain_unit + frame)).read_frame()
    bad = bytearray(grain_unit)
    bad[3] = 3
    with pytest.raises(ValueError, match="corr"):
        B.StreamReader(io.BytesIO(sps + bytes(bad) + frame)).read_frame()
    for cut in range(1, 14):
        with pytest.raises(EOFError):
            B.StreamReader(io.BytesIO(sps + grain_unit[:cut])).read_frame()
    with pytest.raises(EOFError):
        B.StreamReader(io.BytesIO(sps + grain_unit)).read_frame()
    with pytest.raises(ValueError):
        B.write_grain(io.BytesIO(), 16, P1)


def test_stream_without_grain_is_todays_bytes(golden_dir):
    """the reference's own stream (tests/golden/container_kat.json) through packets that carry grain=None"""
    kat = json.load(open(os.path.join(golden_dir, "container_kat.json")))
    rng = np.random.default_rng(5)
    for c in kat["ip"]:                                  # the generator drew the ip payloads first
        rng.integers(0, 256, c["payload_len"], dtype=np.uint8)
    f = io.BytesIO()
    w = B.StreamWriter(f)
    for fr in kat["stream"]["frames"]:
        payload = rng.integers(0, 256, fr["payload_len"], dtype=np.uint8).tobytes()
        w.write_frame(1080, 1920, True, FramePacket(fr["is_i"], fr["qp"], fr["use_ada_i"], payload, grain=None))
    data = f.getvalue()
    assert len(data) == kat["stream"]["n"] and hashlib.sha256(data).hexdigest() == kat["stream"]["sha256"]
    rd = B.StreamReader(io.BytesIO(data))
    for _ in kat["stream"]["frames"]:
        rd.read_frame()
        assert rd.grain is None


# ---------------------------------------------------------------------------------- encoder and command line
class _Net:
    def set_curr_poc(self, poc):
        pass


def test_sequence_encoder_grain_argument():
    assert SequenceEncoder(_Net(), _Net(), 30).grain is None
    assert SequenceEncoder(_Net(), _Net(), 30, grain=P1, defer_stream=True).grain == P1
    est = lambda x, x_hat: None
    assert SequenceEncoder(_Net(), _Net(), 30, grain=est).grain is est
    with pytest.raises(ValueError, match="defer_stream"):
        SequenceEncoder(_Net(), _Net(), 30, grain=est, defer_stream=True)


def test_command_line_and_manifest_options():
    from opendcvc_amd import harness
    ap = harness.build_parser()
    for argv, want in (([], None), (["--film-grain"], "auto"), (["--film_grain"], "auto"), (["--film_grain", "1"], "auto"),
                       (["--film-grain", "0"], None)):
        args = ap.parse_args(["--test-config", "x.json", "--gpus", "1"] + argv)
        opts, _ = harness.manifest_options(args, ap)
        assert opts["film_grain"] == want
