"""The device resampler on the GPU: dcvc_resize_frame against the numpy restatement (tests/resize_ref.py, pinned to Pillow and
torch on the CPU by tests/test_resize_host.py) bit for bit, resize.Resampler, and reduced-resolution coding end to end through
the harness, the container's display unit and a decode loop of the test's own."""
import ctypes
import io

import numpy as np
import pytest
import torch

import resize_ref as R
from opendcvc_amd import _lib, harness, resize, weights
from opendcvc_amd.resize import filter_taps

pytestmark = pytest.mark.gpu

FILTERS = ("bilinear", "bicubic", "lanczos3")
DTYPES = [(torch.float32, np.float32), (torch.float16, np.float16)]
CASES = [((16, 16), (16, 16)),                           # identity tables through the kernel itself
         ((72, 120), (48, 80)), ((48, 80), (72, 120)),   # ratio 1.5
         ((70, 118), (37, 51)), ((37, 51), (70, 118)),   # ratios that differ per axis, odd sizes, an output pad in both directions
         ((64, 64), (8, 8)), ((8, 8), (64, 64)),         # ratio 8: the widest tables (several groups of rows per tile)
         ((270, 480), (180, 320)),                       # many tiles in both directions
         ((33, 40), (20, 24))]                           # a 48 x 48 source tensor, NaN around the picture, rows not 16-byte aligned


def _pad(n, to=16):
    return n + (-n) % to


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint16 if a.dtype == np.float16 else np.uint32)


@pytest.fixture(scope="module")
def sources():
    """per (size, numpy dtype): the picture, uniform in [0, 1), inside a NaN-filled padded tensor - host copy (read-only)
    and device copy, made once"""
    cache = {}

    def get(size, ndt):
        if (size, ndt) not in cache:
            h, w = size
            hp, wp = (48, 48) if size == (33, 40) else (_pad(h), _pad(w))
            host = np.full((3, hp, wp), np.nan, ndt)
            host[:, :h, :w] = np.random.default_rng(h * 1000 + w).random((3, h, w), dtype=np.float32).astype(ndt)
            host.setflags(write=False)
            if size == (33, 40):
                # one element into a larger allocation: no row of the tensor starts 16-byte aligned in fp16
                flat = torch.empty(host.size + 8, dtype=torch.from_numpy(np.zeros(1, ndt)).dtype, device="cuda")
                dev = flat[1:1 + host.size].view(1, 3, hp, wp)
                dev.copy_(torch.from_numpy(np.array(host))[None])
                assert dev.data_ptr() % 16 == host.itemsize and dev.is_contiguous()
            else:
                dev = torch.from_numpy(np.array(host))[None].cuda()
            cache[(size, ndt)] = (host, dev)
        return cache[(size, ndt)]
    yield get
    cache.clear()


def _launch(x, size_in, size_out, th, tv, out=None, taps=None):
    """dcvc_resize_frame itself with host tables th / tv = (first, coef) -> (rc, out [1, 3, HOp, WOp] pre-filled with NaN)"""
    (H, W), (HO, WO) = size_in, size_out
    if out is None:
        out = torch.full((1, 3, _pad(HO), _pad(WO)), float("nan"), dtype=x.dtype, device=x.device)
    dev = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (th[0], th[1], tv[0], tv[1])]
    kh, kv = taps or (th[1].shape[1], tv[1].shape[1])
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = _lib.lib().dcvc_resize_frame(0 if x.dtype == torch.float16 else 1, P(x), x.shape[2], x.shape[3], H, W, P(out), out.shape[2],
                                      out.shape[3], HO, WO, P(dev[0]), P(dev[1]), kh, P(dev[2]), P(dev[3]), kv,
                                      ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, out


# ---------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("tdt,ndt", DTYPES)
@pytest.mark.parametrize("name", FILTERS)
@pytest.mark.parametrize("size_in,size_out", CASES)
def test_kernel_equals_the_restatement(sources, size_in, size_out, name, tdt, ndt):
    host, dev = sources(size_in, ndt)
    th, tv = filter_taps(name, size_in[1], size_out[1]), filter_taps(name, size_in[0], size_out[0])
    want = R.resize_tables_ref(host, size_in, th, tv, (_pad(size_out[0]), _pad(size_out[1])))
    rc, out = _launch(dev, size_in, size_out, th, tv)
    assert rc == 0 and out.dtype == tdt
    got = out[0].cpu().numpy()
    assert np.isfinite(got).all()                                   # every element written, no NaN of the source's pad read
    diff = int((_bits(got) != _bits(want)).sum())
    print(f"{size_in} -> {size_out} {name} {ndt.__name__}: {diff} of {got.size} elements differ")
    assert diff == 0
    HO, WO = size_out
    assert np.array_equal(got[:, HO:, :], np.broadcast_to(got[:, HO - 1:HO, :], got[:, HO:, :].shape))
    assert np.array_equal(got[:, :, WO:], np.broadcast_to(got[:, :, WO - 1:WO], got[:, :, WO:].shape))
    if size_in == size_out:
        assert np.array_equal(_bits(got), _bits(host[:, :HO, :WO]))
    rc, again = _launch(dev, size_in, size_out, th, tv)
    assert rc == 0 and torch.equal(again.view(torch.uint8), out.view(torch.uint8))


@pytest.mark.parametrize("tdt,ndt", DTYPES)
@pytest.mark.parametrize("size_in,size_out", [((70, 118), (37, 51)), ((270, 480), (180, 320))])
def test_out_of_range_first_values_are_clamped(sources, size_in, size_out, tdt, ndt):
    """the clamp is the contract: rows of the tables that start 5 before the picture or 5 behind it read its border (at the
    larger size the windows of the first tile then span more columns than the kernel stages in LDS)"""
    host, dev = sources(size_in, ndt)
    th, tv = [list(filter_taps("bicubic", size_in[k], size_out[k])) for k in (1, 0)]
    for (first, _), n_in in ((th, size_in[1]), (tv, size_in[0])):
        first[0], first[3], first[10], first[-1] = -5, n_in + 5, -5, n_in + 5
    want = R.resize_tables_ref(host, size_in, th, tv, (_pad(size_out[0]), _pad(size_out[1])))
    rc, out = _launch(dev, size_in, size_out, th, tv)
    got = out[0].cpu().numpy()
    assert rc == 0 and np.isfinite(got).all() and np.array_equal(_bits(got), _bits(want))


@pytest.mark.parametrize("tdt,ndt", DTYPES)
def test_kernel_does_not_depend_on_where_the_source_lies(tdt, ndt):
    """a 45 x 77 picture in source frames [3, 48, Wp], Wp 80 and 84, each once on a 16-byte boundary and once one element
    into a larger allocation: Wp 80 on the boundary is staged with wide accesses in fp16 and fp32, Wp 84 only in fp32, the
    view never"""
    size_in, size_out = (45, 77), (30, 52)
    picture = np.random.default_rng(4577).random((3, 45, 77), dtype=np.float32).astype(ndt)
    th, tv = filter_taps("bicubic", 77, 52), filter_taps("bicubic", 45, 30)
    got = []
    for wp in (80, 84):
        host = np.full((3, 48, wp), np.nan, ndt)
        host[:, :45, :77] = picture
        want = R.resize_tables_ref(host, size_in, th, tv, (32, 64))
        for mis in (False, True):
            flat = torch.empty(host.size + 8, dtype=tdt, device="cuda")
            dev = flat[int(mis):int(mis) + host.size].view(1, 3, 48, wp)
            dev.copy_(torch.from_numpy(host)[None])
            assert dev.data_ptr() % 16 == int(mis) * host.itemsize and dev.is_contiguous()
            rc, out = _launch(dev, size_in, size_out, th, tv)
            got.append(out[0].cpu().numpy())
            assert rc == 0 and np.isfinite(got[-1]).all() and np.array_equal(_bits(got[-1]), _bits(want))
    assert all(np.array_equal(_bits(g), _bits(got[0])) for g in got)


def test_refused_call_leaves_the_output_untouched(sources):
    size_in, size_out = (72, 120), (48, 80)
    _, dev = sources(size_in, np.float16)
    th, tv = filter_taps("bilinear", 120, 80), filter_taps("bilinear", 72, 48)
    out = torch.full((1, 3, 48, 80), 7.0, dtype=torch.float16, device="cuda")
    for kw in (dict(taps=(65, 3)), dict(taps=(3, 0))):
        rc, o = _launch(dev, size_in, size_out, th, tv, out=out, **kw)
        assert rc < 0 and b"taps" in _lib.lib().dcvc_last_error() and bool((o == 7.0).all())
    rc, o = _launch(dev, size_in, (49, 80), th, tv, out=out)          # the valid region does not fit the tensor
    assert rc < 0 and bool((o == 7.0).all())


# ---------------------------------------------------------------------------------- Resampler
def test_resampler_caches_tables_returns_its_input_and_follows_the_stream(sources, monkeypatch):
    calls = []
    monkeypatch.setattr(resize, "filter_taps", lambda *a: calls.append(a) or filter_taps(*a))
    host, dev = sources((70, 118), np.float16)
    r = resize.Resampler("cuda:0")
    want = R.resize_ref(host, (70, 118), (37, 51), "lanczos3", pad_to=16)
    a = r.resample(dev, (70, 118), (37, 51))
    assert sorted(calls) == [("lanczos3", 70, 37), ("lanczos3", 118, 51)]
    b = r.resample(dev, (70, 118), (37, 51), "lanczos3")
    assert len(calls) == 2 and tuple(a.shape) == (1, 3, 48, 64) and a.dtype == torch.float16
    assert r.resample(dev, (70, 118), (70, 118)) is dev and len(calls) == 2
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        c = r.resample(dev, (70, 118), (37, 51))
    s.synchronize()
    torch.cuda.synchronize()
    for got in (a, b, c):
        assert np.array_equal(_bits(got[0].cpu().numpy()), _bits(want))
    assert tuple(r.resample(dev, (70, 118), (37, 51), "bilinear", pad_to=8).shape) == (1, 3, 40, 56) and len(calls) == 4
    with pytest.raises(ValueError):
        r.resample(dev, (70, 118), (37, 51), "nearest")


# ---------------------------------------------------------------------------------- end to end
H, W, N, CODED = 96, 128, 8, (64, 80)


@pytest.fixture(scope="module")
def clip(tmp_path_factory):
    """fp32 codecs with the synthetic weights and 8 synthetic 96 x 128 frames as a YUV 4:2:0 file"""
    from opendcvc_amd.models import DMC, DMCI
    nets = []
    for cls, name in ((DMCI, "dmci"), (DMC, "dmc")):
        m = cls()
        m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in weights.make_state_dict(name, 1234).items()})
        m.to("cuda").eval()
        m.update(0.12)
        nets.append(m)
    folder = tmp_path_factory.mktemp("resize")
    src = folder / "clip.yuv"
    frames = [weights.synthetic_frame_yuv420(H, W, i, 3) for i in range(N)]
    with open(src, "wb") as f:
        for planes in frames:
            for plane in planes:
                f.write(plane.tobytes())
    return nets, str(src), frames, folder


def _run(clip, name, **kw):
    nets, src, _, folder = clip
    path = str(folder / f"{name}.bin")
    log = harness.run_one_point(nets[0], nets[1], src, W, H, N, 32, 32, intra_period=4, reset_interval=32, verbose_json=True,
                                metrics="device", bin_path=path, **kw)
    return log, open(path, "rb").read()


def test_reduced_resolution_run_and_a_decoder_of_the_tests_own(clip):
    from opendcvc_amd.bitstream import StreamReader
    from opendcvc_amd.metrics import DeviceMetrics
    from opendcvc_amd.pipeline import FramePacket, SequenceDecoder
    nets, _, frames, _ = clip
    plain, plain_bytes = _run(clip, "plain")
    log, data = _run(clip, "scaled", coded_size=CODED)
    assert list(log) == list(plain) + ["coded_height", "coded_width", "scale_filter"]
    assert (log["coded_height"], log["coded_width"], log["scale_filter"]) == CODED + ("lanczos3",)
    assert log["frame_pixel_num"] == H * W and sum(log["frame_bpp"]) * H * W == pytest.approx(8 * len(data))
    assert all(np.isfinite(v) and 0 < v < 99 for v in log["frame_psnr"]) and len(data) < len(plain_bytes)
    reader = StreamReader(io.BytesIO(data))
    dec, scaler, dm, psnr = None, resize.Resampler("cuda:0"), DeviceMetrics("cuda:0"), []
    for fi in range(N):
        sps, is_i, qp, payload = reader.read_frame()
        assert (sps["height"], sps["width"]) == CODED and reader.display == (H, W, "lanczos3")
        if dec is None:
            dec = SequenceDecoder(nets[0], nets[1], sps["height"], sps["width"], bool(sps["ec_part"]))
        x_hat = dec.decode(FramePacket(is_i, qp, sps["use_ada_i"], payload, chunked=reader.chunked, digest=reader.digest))
        x_hat = scaler.resample(x_hat, CODED, reader.display[:2], reader.display[2])
        assert tuple(x_hat.shape) == (1, 3, H, W)
        y, u, v = (torch.from_numpy(np.array(p)).cuda() for p in frames[fi])
        psnr.append(dm.yuv420(x_hat, y, u, v)[0])
    print("frame PSNR", [p[0] for p in psnr], "log", log["frame_psnr"])
    assert [p[0] for p in psnr] == log["frame_psnr"] and [p[1] for p in psnr] == log["frame_psnr_y"]


def test_the_source_size_as_coded_size_is_the_run_of_today(clip):
    off, off_bytes = _run(clip, "off")
    same, same_bytes = _run(clip, "same", coded_size=(H, W), scale_filter="bicubic")
    assert same_bytes == off_bytes and list(same) == list(off)
    assert {k: v for k, v in same.items() if k != "test_time"} == {k: v for k, v in off.items() if k != "test_time"}


def test_the_options_compose(clip):
    log, data = _run(clip, "all", coded_size=CODED, scale_filter="bicubic", scenecut=150, target_bpp=0.3, digest=True)
    assert log["digests_checked"] == N and log["scale_filter"] == "bicubic" and log["target_bpp"] == 0.3
    assert list(log)[-3:] == ["coded_height", "coded_width", "scale_filter"] and "scene_cuts" in log
    assert sum(log["frame_bpp"]) * H * W == pytest.approx(8 * len(data))
    from opendcvc_amd.bitstream import StreamReader
    reader = StreamReader(io.BytesIO(data))
    for _ in range(N):
        sps, *_ = reader.read_frame()
        assert (sps["height"], sps["width"]) == CODED and reader.display == (H, W, "bicubic") and reader.digest is not None
