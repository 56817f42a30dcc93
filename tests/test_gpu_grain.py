"""Film grain on the GPU (docs/film_grain.md): dcvc_grain_apply and dcvc_grain_stats against the numpy restatement
(tests/grain_ref.py, held against the doc's figures on the CPU by tests/test_grain_host.py) bit for bit, grain.FilmGrain, and
grain units end to end through the harness and a decode loop of the test's own."""
import io

import numpy as np
import pytest
import torch

import grain_ref as G
from opendcvc_amd import bitstream as B
from opendcvc_amd import harness, resize, weights
from opendcvc_amd.grain import FilmGrain, GrainParams, params_from_stats

pytestmark = pytest.mark.gpu

DTYPES = [(torch.float32, np.float32), (torch.float16, np.float16)]
SIZES = [(16, 16),                 # smaller than a tile plus halo
         (33, 40),                 # a 48 x 48 tensor, NaN around the picture, carved one element into a larger allocation
         (70, 118),                # odd sizes, partial tiles on both edges
         (270, 480)]               # many tiles: every seam is compared
SCALE_Y = (8, 40, 72, 104, 136, 168, 200, 255)


def _pad(n, to=16):
    return n + (-n) % to


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint16 if a.dtype == np.float16 else np.uint32)


def _to_device(host, misaligned):
    if not misaligned:
        return torch.from_numpy(np.array(host))[None].cuda()
    flat = torch.empty(host.size + 8, dtype=torch.from_numpy(np.zeros(1, host.dtype)).dtype, device="cuda")
    dev = flat[1:1 + host.size].view(1, *host.shape)
    dev.copy_(torch.from_numpy(np.array(host))[None])
    assert dev.data_ptr() % 16 == host.itemsize and dev.is_contiguous()       # no row starts 16-byte aligned in fp16
    return dev


def _padded_shape(size):
    return (48, 48) if size == (33, 40) else (_pad(size[0]), _pad(size[1]))


@pytest.fixture(scope="module")
def sources():
    """per (size, numpy dtype): a picture uniform in [-0.1, 1.1) inside a NaN-filled padded tensor - host (read-only) and device"""
    cache = {}

    def get(size, ndt):
        if (size, ndt) not in cache:
            h, w = size
            host = np.full((3,) + _padded_shape(size), np.nan, ndt)
            host[:, :h, :w] = (np.random.default_rng(h * 1000 + w).random((3, h, w), dtype=np.float32) * 1.2 - 0.1).astype(ndt)
            host[0, 0, 0] = -0.0
            host.setflags(write=False)
            cache[(size, ndt)] = (host, _to_device(host, size == (33, 40)))
        return cache[(size, ndt)]
    yield get
    cache.clear()


@pytest.fixture(scope="module")
def fg():
    return FilmGrain("cuda:0")


# ---------------------------------------------------------------------------------- dcvc_grain_apply
@pytest.mark.parametrize("tdt,ndt", DTYPES)
@pytest.mark.parametrize("t", [0, 5])
@pytest.mark.parametrize("corr", [0, 1, 2])
@pytest.mark.parametrize("size", SIZES)
def test_apply_equals_the_restatement(sources, fg, size, corr, t, tdt, ndt):
    host, dev = sources(size, ndt)
    p = GrainParams(4242, corr, SCALE_Y, 90, 160)
    want = G.apply(host, size, p.seed, corr, p.scale_y, p.scale_cb, p.scale_cr, t)
    out = torch.full_like(dev, 7.0)
    assert fg.apply(dev, size, p, t, out=out) is out and out.dtype == tdt
    torch.cuda.synchronize()
    got = out[0].cpu().numpy()
    H, W = size
    diff = int((_bits(got) != _bits(want)).sum())
    print(f"{size} corr {corr} t {t} {ndt.__name__}: {diff} of {got.size} elements differ")
    assert diff == 0
    assert np.isfinite(got[:, :H, :W]).all()
    pad = np.ones(got.shape, bool)
    pad[:, :H, :W] = False
    assert np.array_equal(_bits(got)[pad], _bits(host)[pad])                # the pad: the same NaN bits
    assert (_bits(got[:, :H, :W]) != _bits(host[:, :H, :W])).mean() > 0.5      # and it is not the identity
    assert np.array_equal(_bits(dev[0].cpu().numpy()), _bits(host))          # the input is untouched


@pytest.mark.parametrize("tdt,ndt", DTYPES)
@pytest.mark.parametrize("size,corr", [((33, 40), 1), ((270, 480), 2), ((70, 118), 0)])
def test_in_place_equals_out_of_place(sources, fg, size, corr, tdt, ndt):
    _, dev = sources(size, ndt)
    p = GrainParams(17, corr, SCALE_Y, 30, 60)
    apart = fg.apply(dev, size, p, 3)
    work = _to_device(dev[0].cpu().numpy(), size == (33, 40))
    assert fg.apply(work, size, p, 3, out=work) is work
    torch.cuda.synchronize()
    assert np.array_equal(_bits(work[0].cpu().numpy()), _bits(apart[0].cpu().numpy()))


def test_zero_strength_and_refused_calls(sources, fg):
    from opendcvc_amd import _lib
    _, dev = sources((70, 118), np.float16)
    out = fg.apply(dev, (70, 118), GrainParams(seed=3, corr=2), 1)
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int16), dev.view(torch.int16))
    keep = torch.full_like(dev, 7.0)
    with pytest.raises(_lib.DcvcError, match="does not hold"):
        fg.apply(dev, (81, 118), GrainParams(scale_cb=9), 0, out=keep)
    torch.cuda.synchronize()
    assert bool((keep == 7.0).all())
    with pytest.raises(ValueError):
        fg.apply(dev, (70, 118), GrainParams(scale_cb=9), 0, out=keep[:, :, :64])


# ---------------------------------------------------------------------------------- dcvc_grain_stats
def _blocky(size, ndt):
    """a picture of 16 x 16 blocks at random levels, some flat (noise far below the threshold), some not; block (0, 0) flat"""
    h, w = size
    rng = np.random.default_rng(h * 77 + w)
    bh, bw = -(-h // 16), -(-w // 16)
    level = np.kron(rng.random((3, bh, bw), dtype=np.float32) * 0.9 + 0.05, np.ones((16, 16), np.float32))[:, :h, :w]
    rough = rng.random((bh, bw)) < 0.3
    rough[0, 0] = False
    amp = np.kron(np.where(rough, 0.06, 0.002).astype(np.float32), np.ones((16, 16), np.float32))[:h, :w]
    host = np.full((3,) + _padded_shape(size), np.nan, ndt)
    host[:, :h, :w] = (level + amp[None] * (rng.random((3, h, w), dtype=np.float32) - 0.5)).astype(ndt)
    return host


@pytest.fixture(scope="module")
def pairs():
    """per (size, numpy dtype, corr): (clean, noisy) host and device; noisy is the restatement's synthesis"""
    cache = {}

    def get(size, ndt, corr):
        key = (size, ndt, corr)
        if key not in cache:
            clean = G.estimator_picture(ndt) if size == (144, 256) else _blocky(size, ndt)
            noisy = G.apply(clean, size, 808, corr, (24, 32, 40, 48, 56, 64, 72, 80), 36, 52, 0)
            for a in (clean, noisy):
                a.setflags(write=False)
            mis = size == (33, 40)
            cache[key] = (clean, noisy, _to_device(clean, mis), _to_device(noisy, mis))
        return cache[key]
    yield get
    cache.clear()


@pytest.mark.parametrize("tdt,ndt", DTYPES)
@pytest.mark.parametrize("size,corr", [((144, 256), 0), ((144, 256), 2), ((16, 16), 1), ((33, 40), 1), ((270, 480), 2)])
def test_stats_table_equals_the_restatement(pairs, fg, size, corr, tdt, ndt):
    clean, noisy, dclean, dnoisy = pairs(size, ndt, corr)
    want = G.stats(noisy, clean, size)
    got = fg.stats(dnoisy, dclean, size)
    print(f"{size} {ndt.__name__}: counts {got[:, 0].tolist()}")
    assert got.dtype == np.int64 and got.shape == (12, 2) and np.array_equal(got, want)
    blocks = (size[0] // 16) * (size[1] // 16)
    assert blocks == {(144, 256): 144, (16, 16): 1, (33, 40): 4, (270, 480): 480}[size]
    assert 0 < got[8, 0] <= blocks and got[:8, 0].sum() == got[8, 0] == got[11, 0] and got[:8, 1].min() >= 0
    if size == (144, 256):
        assert got[:8, 0].tolist() == [16] * 8              # no checker-strip block
    if size == (270, 480):
        assert got[8, 0] < blocks                           # flat and not flat blocks
    assert np.array_equal(fg.stats(dnoisy, dclean, size), want)          # the call zeroes its table


def test_stats_of_a_picture_below_one_block_is_the_zero_table(pairs, fg):
    _, _, dclean, dnoisy = pairs((16, 16), np.float32, 1)
    assert not fg.stats(dnoisy, dclean, (15, 16)).any()


@pytest.mark.parametrize("tdt,ndt", DTYPES)
@pytest.mark.parametrize("corr", [0, 1, 2])
def test_round_trip_on_the_device(pairs, fg, corr, tdt, ndt):
    clean, noisy, dclean, _ = pairs((144, 256), ndt, corr)
    p = GrainParams(808, corr, (24, 32, 40, 48, 56, 64, 72, 80), 36, 52)
    got = fg.estimate(fg.apply(dclean, (144, 256), p, 0), dclean, (144, 256), 5)
    want = params_from_stats(G.stats(noisy, clean, (144, 256)), 5)
    print(f"corr {corr} {ndt.__name__}: {got}")
    assert got is not None and got == want and got.corr == corr and got.seed == 5


# ---------------------------------------------------------------------------------- where the frame lies
def _placements(picture, fill=np.nan):
    """a 45 x 77 picture in frames [3, 48, Wp], Wp 80 and 84, each once on a 16-byte boundary and once one element into a
    larger allocation: [(host, device)] x 4.  Wp 80 on the boundary takes the wide accesses in fp16 and fp32, Wp 84 only
    in fp32 (apply) or with either type (stats: four elements), the view never"""
    out = []
    for wp in (80, 84):
        host = np.full((3, 48, wp), fill, picture.dtype)
        host[:, :45, :77] = picture
        for mis in (False, True):
            dev = _to_device(host, mis)
            assert mis or dev.data_ptr() % 16 == 0
            out.append((host, dev))
    return out


@pytest.mark.parametrize("tdt,ndt", DTYPES)
def test_apply_and_stats_do_not_depend_on_where_the_frame_lies(fg, tdt, ndt):
    size = (45, 77)
    p = GrainParams(808, 2, (24, 32, 40, 48, 56, 64, 72, 80), 36, 52)
    clean = _blocky(size, ndt)[:, :45, :77]
    pictures, tables = [], []
    for host, dev in _placements(clean):
        want = G.apply(host, size, p.seed, p.corr, p.scale_y, p.scale_cb, p.scale_cr, 3)
        out = _to_device(np.full_like(host, 7.0), dev.data_ptr() % 16 != 0)
        fg.apply(dev, size, p, 3, out=out)
        got = out[0].cpu().numpy()
        assert np.array_equal(_bits(got), _bits(want))
        pictures.append(_bits(got[:, :45, :77]))
        tables.append(fg.stats(out, dev, size))
        assert np.array_equal(tables[-1], G.stats(want, host, size)) and tables[-1][8, 0] > 0
    assert all(np.array_equal(a, pictures[0]) for a in pictures) and all(np.array_equal(t, tables[0]) for t in tables)
    assert (pictures[0] != _bits(clean)).mean() > 0.5


# ---------------------------------------------------------------------------------- end to end
H, W, N, CODED = 64, 96, 8, (48, 64)
PARAMS = GrainParams(1001, 1, (20, 24, 28, 32, 36, 40, 44, 48), 16, 12)


def _write_clip(path, frames):
    with open(path, "wb") as f:
        for planes in frames:
            for plane in planes:
                f.write(plane.tobytes())


@pytest.fixture(scope="module")
def clip(tmp_path_factory):
    """fp32 codecs with the synthetic weights, 8 synthetic 64 x 96 frames as a YUV 4:2:0 file, and the same with grain"""
    from opendcvc_amd.models import DMC, DMCI
    nets = []
    for cls, name in ((DMCI, "dmci"), (DMC, "dmc")):
        m = cls()
        m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in weights.make_state_dict(name, 1234).items()})
        m.to("cuda").eval()
        m.update(0.12)
        nets.append(m)
    folder = tmp_path_factory.mktemp("grain")
    frames = [weights.synthetic_frame_yuv420(H, W, i, 3) for i in range(N)]
    _write_clip(folder / "clip.yuv", frames)
    grainy = []
    for i, planes in enumerate(frames):
        out = []
        for c, plane in enumerate(planes):
            n = G.white(55, i, c, 0, 0, *plane.shape) * (6.0 / np.sqrt(G.VAR_WHITE))          # 6 code values
            out.append(np.clip(np.rint(plane.astype(np.float64) + n), 0, 255).astype(np.uint8))
        grainy.append(tuple(out))
    _write_clip(folder / "grainy.yuv", grainy)
    return nets, folder


def _run(clip, name, src="clip.yuv", **kw):
    nets, folder = clip
    path, rec = str(folder / f"{name}.bin"), str(folder / f"{name}.yuv")
    log = harness.run_one_point(nets[0], nets[1], str(folder / src), W, H, N, 32, 32, intra_period=4, reset_interval=32,
                                verbose_json=True, metrics="device", bin_path=path, rec_path=rec, **kw)
    return log, open(path, "rb").read(), open(rec, "rb").read()


def _unit_types(data):
    """the NAL types of a stream in order, and the grain units' parameters"""
    f, types, grains = io.BytesIO(data), [], []
    while f.tell() < len(data):
        h = B.read_header(f)
        types.append(int(h["nal_type"]))
        if h["nal_type"] == B.NalType.NAL_SPS:
            B.read_sps_remaining(f, h["sps_id"])
        elif h["nal_type"] == B.NalType.NAL_DISPLAY:
            B.read_display_remaining(f)
        elif h["nal_type"] == B.NalType.NAL_DIGEST:
            B.read_digest_remaining(f)
        elif h["nal_type"] == B.NalType.NAL_GRAIN:
            grains.append(B.read_grain_remaining(f))
        else:
            B.read_ip_remaining(f)
    return types, grains


def _decode_with_grain(clip, data, coded=None):
    """a decode loop of the test's own: the stored planes of grain_ref.apply(decoded picture), frame after frame"""
    from opendcvc_amd.pipeline import FramePacket, SequenceDecoder, store_yuv420_frame
    nets, _ = clip
    reader, dec, scaler, out, ts = B.StreamReader(io.BytesIO(data)), None, resize.Resampler("cuda:0"), b"", []
    for _ in range(N):
        sps, is_i, qp, payload = reader.read_frame()
        if dec is None:
            dec = SequenceDecoder(nets[0], nets[1], sps["height"], sps["width"], bool(sps["ec_part"]))
        x_hat = dec.decode(FramePacket(is_i, qp, sps["use_ada_i"], payload, chunked=reader.chunked, digest=reader.digest))
        if coded:
            assert (sps["height"], sps["width"]) == coded and reader.display[:2] == (H, W)
            x_hat = scaler.resample(x_hat, coded, (H, W), reader.display[2])
        g, ts = reader.grain, ts + [reader.grain_t]
        assert g == PARAMS
        host = G.apply(x_hat[0].cpu().numpy(), (H, W), g.seed, g.corr, g.scale_y, g.scale_cb, g.scale_cr, reader.grain_t)
        for plane in store_yuv420_frame(torch.from_numpy(host)[None].cuda(), H, W):
            out += plane.cpu().numpy().tobytes()
    dec.flush()
    assert ts == [0, 1, 2, 3, 0, 1, 2, 3]
    return out


def _metric_keys(log):
    return {k: v for k, v in log.items() if "psnr" in k or "msssim" in k}


@pytest.fixture(scope="module")
def plain(clip):
    return _run(clip, "plain")


def test_fixed_params_through_the_harness(clip, plain):
    log0, data0, rec0 = plain
    log, data, rec = _run(clip, "fixed", film_grain=PARAMS)
    types, grains = _unit_types(data)
    assert grains == [PARAMS, PARAMS] and types.count(1) == 2
    assert all(types[i - 1] == 7 for i, t in enumerate(types) if t == 1)          # in front of each of the two I frames
    assert [t for t in types if t != 7] == _unit_types(data0)[0]
    bits = lambda l: round(sum(l["frame_bpp"]) * H * W)
    assert bits(log) == 8 * len(data) and bits(log) - bits(log0) == 2 * 14 * 8
    assert list(log) == list(log0) + ["grain_units", "grain_scale_y", "grain_corr"]
    assert (log["grain_units"], log["grain_scale_y"], log["grain_corr"]) == (2, list(PARAMS.scale_y), 1)
    assert _metric_keys(log) == _metric_keys(log0) and len(_metric_keys(log)) >= 12          # metrics: before synthesis
    assert rec != rec0 and len(rec) == len(rec0) == N * H * W * 3 // 2
    assert rec == _decode_with_grain(clip, data)


def test_grain_is_applied_behind_the_display_upscale(clip):
    log0, _, _ = _run(clip, "scaled", coded_size=CODED)
    log, data, rec = _run(clip, "scaled_grain", coded_size=CODED, film_grain=PARAMS)
    types, grains = _unit_types(data)
    assert grains == [PARAMS, PARAMS] and all(types[i - 1] == 7 for i, t in enumerate(types) if t == 1)
    assert _metric_keys(log) == _metric_keys(log0)
    assert list(log)[-6:] == ["coded_height", "coded_width", "scale_filter", "grain_units", "grain_scale_y", "grain_corr"]
    assert rec == _decode_with_grain(clip, data, coded=CODED)


def test_unit_order_with_digests_and_the_other_options(clip):
    log, data, rec = _run(clip, "digest", film_grain=PARAMS, digest=True)
    types, grains = _unit_types(data)
    assert grains == [PARAMS, PARAMS] and log["digests_checked"] == N
    for i, t in enumerate(types):
        if t in (1, 2):
            assert types[i - 1] == 5 and (types[i - 2] == 7) == (t == 1)          # grain, digest, I frame
    assert rec == _decode_with_grain(clip, data)
    log, data, _ = _run(clip, "all", film_grain=PARAMS, digest=True, coded_size=CODED, scenecut=150, target_bpp=0.3,
                        entropy="device")
    types, grains = _unit_types(data)
    i_frames = [i for i, t in enumerate(types) if t == 3]
    assert len(grains) == len(i_frames) == log["grain_units"] and all(types[i - 2:i] == [7, 5] for i in i_frames)
    assert round(sum(log["frame_bpp"]) * H * W) == 8 * len(data)


def test_an_estimator_callable_is_asked_at_every_i_frame(clip, pairs, fg):
    """SequenceEncoder(grain=callable): called with the encoder's input and the I frame's reconstruction, its answer rides on
    the I frame's packet.  The callable here measures the input against the clean picture it knows, so the answer is the
    restatement's (the reconstruction of the synthetic weights is no yardstick)."""
    from opendcvc_amd.pipeline import SequenceEncoder, use_two_entropy_coders
    nets, _ = clip
    clean, noisy, dclean, dnoisy = pairs((144, 256), np.float32, 1)
    want = params_from_stats(G.stats(noisy, clean, (144, 256)), 0)
    assert want is not None and want.corr == 1
    seen = []

    def estimate(x, x_hat):
        assert x is dnoisy and x_hat.shape == x.shape and x_hat.dtype == x.dtype
        seen.append(len(seen))
        return fg.estimate(x, dclean, (144, 256), 0) if len(seen) < 3 else None
    for m in nets:
        m.set_use_two_entropy_coders(use_two_entropy_coders(144, 256))
    enc = SequenceEncoder(nets[0], nets[1], 32, 32, intra_period=2, grain=estimate)
    pkts = [enc.encode(dnoisy) for _ in range(6)]
    assert [p.is_i for p in pkts] == [True, False] * 3 and seen == [0, 1, 2]
    assert [p.grain for p in pkts] == [want, None, want, None, None, None] and enc.grain_units == [want, want]


def test_film_grain_none_is_the_run_of_today(clip, plain):
    log0, data0, rec0 = plain
    log, data, rec = _run(clip, "none", film_grain=None)
    assert data == data0 and rec == rec0 and list(log) == list(log0)
    assert {k: v for k, v in log.items() if k != "test_time"} == {k: v for k, v in log0.items() if k != "test_time"}
    with pytest.raises(ValueError):
        _run(clip, "bad", film_grain="on")


def test_auto_estimates_and_writes_valid_units(clip):
    """with the synthetic weights nothing is claimed about the values: the run completes, the units parse, the log has its keys"""
    for name, kw in (("auto", {}), ("auto_scaled", dict(coded_size=CODED))):
        log, data, rec = _run(clip, name, src="grainy.yuv", film_grain="auto", **kw)
        types, grains = _unit_types(data)
        print(name, log["grain_units"], log["grain_scale_y"], log["grain_corr"], grains)
        assert log["grain_units"] == len(grains) <= 2 and all(isinstance(g, GrainParams) and g.active for g in grains)
        assert list(log)[-3:] == ["grain_units", "grain_scale_y", "grain_corr"] and log["grain_corr"] in (0, 1, 2)
        assert log["grain_scale_y"] == (list(grains[-1].scale_y) if grains else [])
        assert all(g.seed in (0, 4) for g in grains)                     # the I frames' indices
        assert round(sum(log["frame_bpp"]) * H * W) == 8 * len(data) and len(rec) == N * H * W * 3 // 2
