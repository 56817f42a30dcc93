"""High-bit-depth, 4:4:4 and NV12 / P010 frame I/O on the device (csrc/dcvc_pixfmt.hip, pipeline.load_frame / store_frame,
metrics.DeviceMetrics.yuv): bit for bit against the planes the reference family's reader / writer produced
(tests/golden/frame_io_hbd.npz, tests/golden/make_golden_pixfmt.py) and against the numpy restatement tests/pixfmt_ref.py
(pinned to that fixture on the CPU by tests/test_pixfmt_host.py) at real sizes; the equivalences that tie the new formats
to the pinned 8-bit path; the device metrics against the harness's host path; whole rate points."""
import os

import numpy as np
import pytest
import torch

import pixfmt_ref as R
from opendcvc_amd import harness, weights
from opendcvc_amd.metrics import DeviceMetrics
from opendcvc_amd.pipeline import PixelFormat, load_frame, load_yuv420_frame, store_frame

pytestmark = pytest.mark.gpu

DTYPES = [(torch.float32, np.float32, "f32"), (torch.float16, np.float16, "f16")]
SIZES = [(1080, 1920), (70, 98)]                     # full size; odd half-width, width not a multiple of 8
YUV420P = PixelFormat("yuv420p", 420, 8)             # planar 8-bit 4:2:0 THROUGH THE NEW KERNELS (the comparator of nv12's
#                                                      store; the src_type "yuv420" keeps its own kernels and arithmetic)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(planes):
    return [p.cpu().numpy() for p in planes]


def _planar(chroma, bits):
    return YUV420P if (chroma, bits) == (420, 8) else PixelFormat.parse(f"yuv{chroma}p" + ("" if bits == 8 else f"{bits}le"))


def _random_planes(rng, h, w, chroma, bits):
    ch, cw = (h, w) if chroma == 444 else (h // 2, w // 2)
    planes = [rng.integers(0, 1 << bits, s).astype(R.sample_dtype(bits)) for s in ((h, w), (ch, cw), (ch, cw))]
    planes[0][0, :2] = (0, (1 << bits) - 1)
    return planes


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "frame_io_hbd.npz"))


# --------------------------------------------------------------------------------------------- 1. the reference's planes
@pytest.mark.parametrize("tdt,ndt,name", DTYPES)
@pytest.mark.parametrize("tag,chroma,bits", R.CASES)
def test_load_matches_the_reference_reader(gold, tag, chroma, bits, tdt, ndt, name):
    want = gold[f"frame_{tag}_{chroma}_{bits}"].astype(ndt)
    _, h, w = want.shape
    planes = R.fixture_source(gold, tag, chroma, bits)
    got = load_frame([_dev(p) for p in planes], _planar(chroma, bits), tdt)
    assert got.dtype == tdt and tuple(got.shape) == (1, 3, h + (-h) % 16, w + (-w) % 16)
    g = got.cpu().numpy()
    assert np.array_equal(g[0, :, :h, :w], want)
    assert np.array_equal(g[0, :, h:, :], np.broadcast_to(g[0, :, h - 1:h, :], g[0, :, h:, :].shape))
    assert np.array_equal(g[0, :, :, w:], np.broadcast_to(g[0, :, :, w - 1:w], g[0, :, :, w:].shape))
    assert np.array_equal(g, R.load_ref(planes, chroma, bits, ndt))


@pytest.mark.parametrize("tdt,ndt,name", DTYPES)
@pytest.mark.parametrize("tag,chroma,bits", R.CASES)
def test_store_matches_the_reference_writer(gold, tag, chroma, bits, tdt, ndt, name):
    x, h, w = R.fixture_reconstruction(gold, tag, ndt)
    got = store_frame(_dev(x), h, w, _planar(chroma, bits))
    assert len(got) == 3
    for g, want, k in zip(_host(got), R.fixture_written(gold, tag, chroma, bits, name), "yuv"):
        assert g.dtype == np.uint16 and g.shape == want.shape
        assert np.array_equal(g, want), (k, int((g != want).sum()))


# --------------------------------------------------------------------------------------------- 2. equivalences
@pytest.mark.parametrize("tdt,ndt,name", DTYPES)
@pytest.mark.parametrize("h,w", SIZES)
def test_nv12_load_is_the_8_bit_loader_and_p010_the_10_bit_one(h, w, tdt, ndt, name):
    rng = np.random.default_rng(h + w)
    y, u, v = _random_planes(rng, h, w, 420, 8)
    want = load_yuv420_frame(_dev(y), _dev(u), _dev(v), tdt)             # dcvc_yuv420_to_frame, the pinned 8-bit path
    got = load_frame([_dev(y), _dev(R.interleave(u, v))], "nv12", tdt)
    assert got.dtype == tdt and torch.equal(got, want)
    assert torch.equal(load_frame([_dev(p) for p in (y, u, v)], YUV420P, tdt), want)
    y, u, v = _random_planes(rng, h, w, 420, 10)
    want = load_frame([_dev(p) for p in (y, u, v)], "yuv420p10le", tdt)
    low = rng.integers(0, 64, y.shape).astype(np.uint16)                 # (the bits below the sample are ignored)
    got = load_frame([_dev((y << 6) | low), _dev(R.interleave(u, v) << 6)], "p010le", tdt)
    assert torch.equal(got, want)
    assert np.array_equal(want.cpu().numpy(), R.load_ref([y, u, v], 420, 10, ndt))


@pytest.mark.parametrize("tdt,ndt,name", DTYPES)
@pytest.mark.parametrize("h,w", SIZES)
def test_semi_planar_store_is_the_interleaved_planar_store(h, w, tdt, ndt, name):
    rng = np.random.default_rng(h * w)
    x = rng.uniform(-0.05, 1.05, (1, 3, h + (-h) % 16, w + (-w) % 16)).astype(np.float32).astype(ndt)
    xd = _dev(x)
    for semi, planar, bits, shift in (("nv12", YUV420P, 8, 0), ("p010le", "yuv420p10le", 10, 6)):
        y, u, v = _host(store_frame(xd, h, w, planar))
        for g, want in zip((y, u, v), R.store_ref(x, h, w, 420, bits)):
            assert g.dtype == want.dtype and np.array_equal(g, want)
        ys, uvs = _host(store_frame(xd, h, w, semi))
        assert uvs.shape == (h // 2, w)
        assert np.array_equal(ys, y << shift) and np.array_equal(uvs, R.interleave(u, v) << shift)


@pytest.mark.parametrize("fmt,pitch", [("yuv420p10le", (24, 12)), ("yuv420p10le", (3, 1)), ("yuv444p", (5, 5)), ("nv12", (6, 6)),
                                       ("p010le", (2, 2)), ("yuv444p16le", (8, 8))])
@pytest.mark.parametrize("h,w", SIZES)
def test_pitched_source_equals_the_tight_one(h, w, fmt, pitch):
    """rows with a pitch (whatever access width the pitch allows) are read in place"""
    f = PixelFormat.parse(fmt)
    rng = np.random.default_rng(7)
    shapes = f.plane_shapes(h, w)
    tight = [rng.integers(0, 1 << (16 if f.msb_aligned else f.bit_depth), s).astype(f.numpy_dtype) for s in shapes]
    padded = []
    for k, p in enumerate(tight):
        q = rng.integers(0, 256, (p.shape[0], p.shape[1] + pitch[min(k, 1)])).astype(p.dtype)      # (junk in the pitch)
        q[:, :p.shape[1]] = p
        padded.append(_dev(q))
    for tdt, _, _ in DTYPES:
        want = load_frame([_dev(p) for p in tight], f, tdt)
        got = load_frame(padded, f, tdt, height=h, width=w, strides=(shapes[0][1] + pitch[0], shapes[1][1] + pitch[1]))
        assert torch.equal(got, want)


@pytest.mark.parametrize("h,w", SIZES)
def test_444_8_bit_load_is_the_quotient_cast(h, w):
    planes = _random_planes(np.random.default_rng(3), h, w, 444, 8)
    for tdt, ndt, _ in DTYPES:
        got = load_frame([_dev(p) for p in planes], "yuv444p", tdt).cpu().numpy()
        want = (np.stack(planes).astype(np.float32) / np.float32(255)).astype(ndt)
        assert np.array_equal(got[0, :, :h, :w], want) and np.array_equal(got, R.load_ref(planes, 444, 8, ndt))


@pytest.mark.parametrize("chroma", [420, 444])
@pytest.mark.parametrize("bits", [8, 10, 12, 16])
@pytest.mark.parametrize("h,w", SIZES)
def test_round_trip(h, w, bits, chroma):
    """planes -> frame -> planes.  fp32 (24 significand bits): the source comes back at every bit depth.  fp16 has 11
    significand bits, so every 8- and 10-bit sample / max_val survives the rounding well enough to be rounded back (zero
    differing samples), 12- and 16-bit samples do not in general: there the returned sample is off by no more than the
    fp16 rounding of the quotient (half an fp16 ulp of it, scaled by max_val) plus the half of the final rounding."""
    fmt = _planar(chroma, bits)
    planes = _random_planes(np.random.default_rng(bits), h, w, chroma, bits)
    dev = [_dev(p) for p in planes]
    back = _host(store_frame(load_frame(dev, fmt, torch.float32), h, w, fmt))
    for b, p in zip(back, planes):
        assert b.dtype == p.dtype and np.array_equal(b, p)
    back = _host(store_frame(load_frame(dev, fmt, torch.float16), h, w, fmt))
    max_val = (1 << bits) - 1
    for b, p in zip(back, planes):
        differing = int((b != p).sum())
        print(f"round trip fp16 {fmt.name} {h}x{w}: {differing} of {p.size} samples differ")
        if bits <= 10:
            assert differing == 0
        else:
            q = (p.astype(np.float32) / np.float32(max_val)).astype(np.float16)
            bound = 0.5 * np.spacing(q).astype(np.float64) * max_val + 0.5
            assert np.all(np.abs(b.astype(np.float64) - p.astype(np.float64)) <= bound)


@pytest.mark.parametrize("tdt,ndt,name", DTYPES)
@pytest.mark.parametrize("fmt", ["yuv420p12le", "yuv444p10le", "yuv420p16le", "yuv444p16le", "yuv444p"])
def test_store_at_1080p_equals_the_restatement(fmt, tdt, ndt, name):
    f = PixelFormat.parse(fmt)
    h, w = 1080, 1920
    x = np.random.default_rng(f.bit_depth).uniform(-0.05, 1.05, (1, 3, 1088, 1920)).astype(np.float32).astype(ndt)
    for g, want in zip(_host(store_frame(_dev(x), h, w, f)), R.store_ref(x, h, w, f.chroma, f.bit_depth)):
        assert g.dtype == want.dtype and np.array_equal(g, want)


# --------------------------------------------------------------------------------------------- 3. metrics
@pytest.fixture(scope="module")
def dm():
    return DeviceMetrics("cuda:0")


def _smooth_source(rng, h, w, fmt):
    yy, xx = np.mgrid[:h, :w]
    full = [np.clip(((np.sin(xx / 17. + k) + np.cos(yy / 29.)) * 0.23 + 0.5) * fmt.max_val + rng.normal(0, fmt.max_val / 32, (h, w)),
                    0, fmt.max_val).astype(fmt.numpy_dtype) for k in range(3)]
    if fmt.chroma == 420:
        full = [full[0], np.ascontiguousarray(full[1][::2, ::2]), np.ascontiguousarray(full[2][::2, ::2])]
    return full


@pytest.mark.parametrize("tdt,ndt,name", DTYPES)
@pytest.mark.parametrize("fmt", ["yuv420p10le", "yuv420p12le", "yuv444p10le", "yuv444p12le"])
@pytest.mark.parametrize("h,w", [(88, 88), (176, 208), (1080, 1920)])
def test_device_metrics_match_the_host_path(dm, h, w, fmt, tdt, ndt, name):
    """DeviceMetrics.yuv against harness.pixfmt_distortion on the same tensors: PSNR within 1e-9 dB, MS-SSIM within 1e-12 on
    all three planes (both paths compare the same fp32 planes).  MS-SSIM where every plane has at least 88 x 88 samples."""
    f = PixelFormat.parse(fmt)
    rng = np.random.default_rng(h + f.bit_depth)
    planes = [_dev(p) for p in _smooth_source(rng, h, w, f)]
    x = load_frame(planes, f, tdt)
    x = (x + _dev(rng.normal(0, 0.01, tuple(x.shape)).astype(np.float32)).to(tdt)).contiguous()
    ssim = min(planes[1].shape) >= 88
    rec = dm.metric_planes(x, h, w, f)
    for g, want in zip(_host(rec), R.metric_planes_ref(x.cpu().numpy(), h, w, f.chroma, f.bit_depth)):
        assert g.dtype == np.float32 and np.array_equal(g, want)
    got_p, got_s = dm.yuv(x, planes, f, calc_ssim=ssim)
    want_p, want_s = harness.pixfmt_distortion(x, planes, f, calc_ssim=ssim)
    for k in range(4):
        print(f"{fmt} {h}x{w} {name} [{k}]: psnr {got_p[k]:.6f} diff {got_p[k] - want_p[k]:.3e}, msssim diff {got_s[k] - want_s[k]:.3e}")
    for k in range(4):
        assert 20 < want_p[k] < 60 and abs(got_p[k] - want_p[k]) <= 1e-9
        assert abs(got_s[k] - want_s[k]) <= 1e-12 and (want_s[k] > 0.5 if ssim else got_s[k] == 0.0)
    assert dm.yuv(x, planes, f, calc_ssim=ssim) == (got_p, got_s)


def test_device_metrics_of_a_p010_source_equal_the_planar_ones(dm):
    f10, fp = PixelFormat.parse("yuv420p10le"), PixelFormat.parse("p010le")
    h, w = 176, 208
    rng = np.random.default_rng(1)
    y, u, v = _smooth_source(rng, h, w, f10)
    x = load_frame([_dev(p) for p in (y, u, v)], f10, torch.float16)
    x = (x + _dev(rng.normal(0, 0.01, tuple(x.shape)).astype(np.float32)).half()).contiguous()
    want = dm.yuv(x, [_dev(p) for p in (y, u, v)], f10, calc_ssim=True)
    semi = [_dev(y << 6), _dev(R.interleave(u, v) << 6)]
    assert dm.yuv(x, semi, fp, calc_ssim=True) == want
    host = harness.pixfmt_distortion(x, semi, fp, calc_ssim=True)
    assert all(abs(a - b) <= 1e-9 for a, b in zip(want[0], host[0])) and all(abs(a - b) <= 1e-12 for a, b in zip(want[1], host[1]))


@pytest.mark.parametrize("n", [1, 257, 1025, 960 * 540 + 1, 1920 * 1080, 3840 * 2160])
def test_sse_with_16_bit_operands_against_numpy(dm, n):
    """relative error <= 1e-9 (the bound test_sse_against_numpy uses for uint8 operands); two runs give the same double"""
    rng = np.random.default_rng(n)
    src = rng.integers(0, 65536, n).astype(np.uint16)
    src[0] = 65535
    rec = np.clip(src + rng.normal(0, 300.0, n), 0, 65535)
    forms = {"u16": src, "f32": rec.astype(np.float32), "u16b": np.rint(rec).astype(np.uint16), "i16view": src.view(np.int16)}
    for ka, kb in (("u16", "f32"), ("u16", "u16b"), ("f32", "u16"), ("i16view", "f32")):
        a, b = forms[ka], forms[kb]
        want = float(np.sum((forms["u16" if ka == "i16view" else ka].astype(np.float64) - b.astype(np.float64)) ** 2))
        ta, tb = _dev(a), _dev(b)
        got = dm.sse(ta, tb)
        print(f"sse n={n} {ka}/{kb}: got {got!r} want {want!r}")
        assert abs(got - want) <= 1e-9 * want, (ka, kb, got, want)
        assert dm.sse(ta, tb) == got


# --------------------------------------------------------------------------------------------- 4. whole rate points
def _nets(mode):
    from opendcvc_amd.models import DMC, DMCI
    nets = []
    for cls, name in ((DMCI, "dmci"), (DMC, "dmc")):
        m = cls()
        m.load_state_dict({k: torch.from_numpy(v) for k, v in weights.make_state_dict(name, 1234).items()})
        m.to("cuda").eval()
        m.update(0.12)
        nets.append(m.half() if mode == "fp16" else m)
    return nets


H, W, N, QP = 136, 200, 6, 24
# Y PSNR of a 16-bit / NV12 copy of an 8-bit clip against the 8-bit run, fp16 model: the 8-bit path compares planes rounded
# to fp16 (clamp(x * 255) in the storage type), the new formats fp32 planes.  Measured on an MI355X (this clip, 6 frames,
# Y PSNR 6.5 .. 6.8 dB with the synthetic weights): 1.799e-05 dB for both the 16-bit and the NV12 copy; the bound is twice
# the measured value ("Raw formats beyond 8-bit 4:2:0").
FP16_Y_PSNR_MEASURED = 1.8e-5
FP16_Y_PSNR_BOUND = 2 * FP16_Y_PSNR_MEASURED


def _write(path, frames):
    with open(path, "wb") as f:
        for planes in frames:
            for p in planes:
                f.write(np.ascontiguousarray(p).tobytes())
    return str(path)


@pytest.mark.parametrize("mode", ["fp32", "fp16"])
def test_16_bit_and_nv12_copies_of_an_8_bit_clip_code_identically(tmp_path, mode):
    """s16 = 257 * s8 gives s16 / 65535 == s8 / 255 in fp32 and NV12 holds the same samples: the same model input bits, so
    the same packets and a byte-identical container; Y PSNR as the metric-plane rule allows"""
    clip = [weights.synthetic_frame_yuv420(H, W, fi, 0) for fi in range(N)]
    src8 = _write(tmp_path / "s8.yuv", clip)
    src16 = _write(tmp_path / "s16.yuv", [[p.astype("<u2") * 257 for p in planes] for planes in clip])
    nv12 = _write(tmp_path / "nv12.yuv", [[y, R.interleave(u, v)] for y, u, v in clip])
    i_net, p_net = _nets(mode)
    logs, bins = {}, {}
    for name, path in (("yuv420", src8), ("yuv420p16le", src16), ("nv12", nv12)):
        bin_path = str(tmp_path / f"{name}.bin")
        logs[name] = harness.run_one_point(i_net, p_net, path, W, H, N, QP, verbose_json=True, src_type=name, bin_path=bin_path)
        bins[name] = open(bin_path, "rb").read()
    ref = logs["yuv420"]
    assert ref["frame_type"] == [0] + [1] * (N - 1) and len(bins["yuv420"]) > 0
    worst = 0.0
    for name in ("yuv420p16le", "nv12"):
        assert bins[name] == bins["yuv420"], f"{name}: container differs from the 8-bit run's"
        assert logs[name]["frame_type"] == ref["frame_type"] and logs[name]["frame_bpp"] == ref["frame_bpp"]
        assert list(logs[name].keys()) == list(ref.keys())
        d = max(abs(a - b) for a, b in zip(logs[name]["frame_psnr_y"], ref["frame_psnr_y"]))
        print(f"{mode} {name}: largest |Y PSNR - 8-bit run's| = {d:.3e} dB (Y PSNR {ref['frame_psnr_y'][0]:.3f} .. {ref['frame_psnr_y'][-1]:.3f})")
        worst = max(worst, d)
    if mode == "fp32":
        assert worst <= 1e-9
    else:
        assert worst <= FP16_Y_PSNR_BOUND


@pytest.mark.parametrize("mode", ["fp32", "fp16"])
def test_a_genuine_10_bit_clip(tmp_path, mode, monkeypatch):
    """4 * s8 + r, r uniform in 0 .. 3: decodes, finite PSNR, the written reconstruction is store_frame of every decoded
    frame (frames * H * W * 3 bytes), metrics="device" and "host" agree within 1e-9 dB"""
    f = PixelFormat.parse("yuv420p10le")
    rng = np.random.default_rng(10)
    clip = [[p.astype("<u2") * 4 + rng.integers(0, 4, p.shape).astype("<u2") for p in weights.synthetic_frame_yuv420(H, W, fi, 0)]
            for fi in range(N)]
    assert any(int((p & 3).max()) == 3 for p in clip[0])
    src = _write(tmp_path / "s10.yuv", clip)
    i_net, p_net = _nets(mode)
    frames, host_fn = [], harness.pixfmt_distortion
    monkeypatch.setattr(harness, "pixfmt_distortion", lambda x_hat, *a, **kw: frames.append(x_hat.clone()) or host_fn(x_hat, *a, **kw))
    rec_path = str(tmp_path / "rec.yuv")
    host = harness.run_one_point(i_net, p_net, src, W, H, N, QP, verbose_json=True, src_type="yuv420p10le", rec_path=rec_path)
    assert len(frames) == N and host["frame_type"] == [0] + [1] * (N - 1)
    assert all(np.isfinite(v) and 0 < v < 99 for k in      # (the synthetic weights reconstruct poorly: a few dB)
               ("frame_psnr", "frame_psnr_y", "frame_psnr_u", "frame_psnr_v") for v in host[k])
    written = open(rec_path, "rb").read()
    assert len(written) == N * H * W * 3 == N * f.frame_bytes(H, W)
    want = b"".join(p.cpu().numpy().tobytes() for x in frames for p in store_frame(x, H, W, f))
    assert written == want
    planes = R.split_planes(np.frombuffer(written, "<u2")[:H * W * 3 // 2], H, W, 420)
    for g, r in zip(planes, R.store_ref(frames[0].cpu().numpy(), H, W, 420, 10)):
        assert np.array_equal(g, r)
    assert max(int(p.max()) for p in planes) <= 1023
    dev = harness.run_one_point(i_net, p_net, src, W, H, N, QP, verbose_json=True, src_type="yuv420p10le", metrics="device")
    assert dev["frame_bpp"] == host["frame_bpp"] and list(dev.keys()) == list(host.keys())
    for k in ("frame_psnr", "frame_psnr_y", "frame_psnr_u", "frame_psnr_v"):
        d = max(abs(a - b) for a, b in zip(dev[k], host[k]))
        print(f"{mode} 10-bit clip {k}: device - host <= {d:.3e} dB")
        assert d <= 1e-9
    assert dev["frame_msssim"] == host["frame_msssim"] == [0.0] * N
