"""Device-side PSNR / MS-SSIM (csrc/dcvc_metrics.hip, opendcvc_amd/metrics.py): metric planes bit for bit, the squared error
against numpy, MS-SSIM against the reference's stored values and against the host path (harness.calc_msssim) at real sizes,
whole rate points with `metrics="device"` against the reference's logs and against `metrics="host"`, and no torch work on
the device path."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from opendcvc_amd import harness
from opendcvc_amd.metrics import DeviceMetrics

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dm():
    return DeviceMetrics("cuda:0")


# --------------------------------------------------------------------------------------------- 1. planes
def _planes_numpy(x, h, w):
    """the stated arithmetic in numpy: every float32 operation on its own (no contraction), each result rounded to the
    storage type"""
    t, f = x.dtype.type, np.float32
    x = x[0, :, :h, :w].astype(f)
    y = np.clip((x[0] * f(255)).astype(t), 0, 255)
    a, b, d, e = x[1:, 0::2, 0::2], x[1:, 0::2, 1::2], x[1:, 1::2, 0::2], x[1:, 1::2, 1::2]
    m = (((a + b) + (d + e)) * f(0.25)).astype(t)
    uv = np.clip((m.astype(f) * f(255)).astype(t), 0, 255)
    return y, uv[0], uv[1]


@pytest.mark.parametrize("name", ["f32", "f16"])
@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_metric_planes_bit_for_bit(dm, golden_dir, tag, name):
    gold = np.load(os.path.join(golden_dir, "frame_io.npz"))
    x = gold[f"rec_{tag}_{name}_x"]
    h, w = gold[f"rec_{tag}_{name}_y"].shape
    got = [p.cpu().numpy() for p in dm.yuv420_planes(torch.from_numpy(x).cuda(), h, w)]
    for g, want, k in zip(got, _planes_numpy(x, h, w), "yuv"):
        assert g.dtype == x.dtype and np.array_equal(g, want), k
    # rounded (Y) / truncated (U, V) they are the reference's 8-bit planes
    assert np.array_equal(np.rint(got[0].astype(np.float32)).astype(np.uint8), gold[f"rec_{tag}_{name}_y"])
    for g, k in ((got[1], "u"), (got[2], "v")):
        assert np.array_equal(g.astype(np.float32).astype(np.uint8), gold[f"rec_{tag}_{name}_{k}"]), k


@pytest.mark.parametrize("dtype", [np.float32, np.float16])
def test_metric_planes_at_1080p(dm, dtype):
    x = np.random.default_rng(11).uniform(-0.1, 1.1, (1, 3, 1088, 1920)).astype(np.float32).astype(dtype)
    got = dm.yuv420_planes(torch.from_numpy(x).cuda(), 1080, 1920)
    for g, want, k in zip(got, _planes_numpy(x, 1080, 1920), "yuv"):
        assert np.array_equal(g.cpu().numpy(), want), k


# --------------------------------------------------------------------------------------------- 2. squared error
@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 1023, 1025, 4 * 256 * 1024 + 3, 1920 * 1080, 960 * 540 + 1, 3840 * 2160])
def test_sse_against_numpy(dm, n):
    """relative error <= 1e-9: n * 2^-53 for 8.3e6 terms of one sign is 9e-10 in the worst case, a tree sum is far below;
    two runs give the identical double (fixed reduction order)"""
    rng = np.random.default_rng(n)
    src = rng.integers(0, 256, n, dtype=np.uint8)
    rec = np.clip(src + rng.normal(0, 5.0, n), 0, 255)
    forms = {"u8": src, "f32": rec.astype(np.float32), "f16": rec.astype(np.float16),
             "u8b": np.rint(rec).astype(np.uint8)}
    for ka, kb in (("u8", "f32"), ("u8", "f16"), ("u8", "u8b"), ("f32", "f16"), ("f16", "u8")):
        a, b = forms[ka], forms[kb]
        want = float(np.sum((a.astype(np.float64) - b.astype(np.float64)) ** 2))
        ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
        got = dm.sse(ta, tb)
        print(f"sse n={n} {ka}/{kb}: got {got!r} want {want!r}")
        assert abs(got - want) <= 1e-9 * want, (ka, kb, got, want)
        assert dm.sse(ta, tb) == got


# --------------------------------------------------------------------------------------------- 3. reference values
def test_msssim_matches_reference_values(dm, golden_dir):
    g = np.load(os.path.join(golden_dir, "frame_io_rgb.npz"))
    for tag in ("l5", "l4", "edge"):
        got = dm.msssim(torch.from_numpy(g[f"ms_{tag}_a"]).cuda(), torch.from_numpy(g[f"ms_{tag}_b"]).cuda())
        print(f"ms_{tag}: device - reference = {got - float(g[f'ms_{tag}_val']):.3e}")
        assert got == pytest.approx(float(g[f"ms_{tag}_val"]), abs=1e-12)
    src = torch.from_numpy(g["src_c_rgb"]).cuda()
    for name in ("f32", "f16"):
        rec = torch.from_numpy(g[f"rec_c_{name}_rgb"]).cuda()
        got = sum(dm.msssim(src[i], rec[i]) for i in range(3)) / 3
        print(f"rgb {name}: device - reference = {got - float(g[f'rec_c_{name}_msssim']):.3e}")
        assert got == pytest.approx(float(g[f"rec_c_{name}_msssim"]), abs=1e-12)


# --------------------------------------------------------------------------------------------- 4. host path, real sizes
def _host_stats(a, b):
    """the per-level means harness.calc_msssim forms (its own helpers, its own loop)"""
    from scipy import ndimage
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    ssim, cs = [], []
    for _ in range(5 if min(a.shape) >= 176 else 4):
        s_map, c_map = harness._ssim_and_cs(a, b, harness._gauss_window(), 255)
        ssim.append(s_map.mean())
        cs.append(c_map.mean())
        a = ndimage.convolve(a, np.full((2, 2), 0.25), mode="reflect")[::2, ::2]
        b = ndimage.convolve(b, np.full((2, 2), 0.25), mode="reflect")[::2, ::2]
    return np.asarray(ssim), np.asarray(cs)


def _smooth_plus_noise(shape, rng):
    yy, xx = np.mgrid[:shape[0], :shape[1]]
    return ((np.sin(xx / 17.) + np.cos(yy / 29.)) * 60 + 128 + rng.normal(0, 8, shape)).clip(0, 255).astype(np.uint8)


@pytest.mark.parametrize("shape", [(1080, 1920), (540, 960), (177, 201), (89, 333), (176, 176), (88, 88)])
def test_msssim_matches_host_path(dm, shape):
    rng = np.random.default_rng(shape[0] * 10000 + shape[1])
    a = _smooth_plus_noise(shape, rng)
    ta = torch.from_numpy(a).cuda()
    for dt, sigma in ((np.float16, 4.0), (np.float32, 4.0), (np.float32, 0.5), (np.float16, 40.0)):
        b = np.clip(a + rng.normal(0, sigma, shape), 0, 255).astype(dt)
        tb = torch.from_numpy(b).cuda()
        ssim, cs = dm.msssim_stats(ta, tb)
        h_ssim, h_cs = _host_stats(a, b)
        want = harness.calc_msssim(a, b.astype(np.float64))
        got = dm.msssim(ta, tb)
        print(f"{shape} {dt.__name__} sigma {sigma}: msssim diff {got - want:.3e}, level means max diff "
              f"{max(np.abs(ssim - h_ssim).max(), np.abs(cs - h_cs).max()):.3e}")
        assert len(ssim) == len(h_ssim) == (5 if min(shape) >= 176 else 4)
        assert np.abs(ssim - h_ssim).max() <= 1e-12 and np.abs(cs - h_cs).max() <= 1e-12
        assert got == pytest.approx(want, abs=1e-12)


def test_msssim_edge_inputs(dm):
    from opendcvc_amd import _lib
    rng = np.random.default_rng(7)
    small = torch.zeros((87, 200), dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError):
        dm.msssim(small, small)
    assert _lib.lib().dcvc_msssim_ws_bytes(87, 200) == -1
    for shape in ((88, 88), (176, 176), (540, 960)):
        a = _smooth_plus_noise(shape, rng)
        ta = torch.from_numpy(a).cuda()
        # a plane against itself: 1.0, and a zero squared error (PSNR capped at 99.9)
        assert dm.msssim(ta, ta) == pytest.approx(1.0, abs=1e-12)
        assert dm.sse(ta, ta) == 0.0 and harness.psnr_from_mse(dm.sse(ta, ta) / a.size) == 99.9
        # against its inverse the contrast means are negative: NaN on both paths; two unrelated noise planes are not NaN
        inv = 255 - a
        assert np.isnan(harness.calc_msssim(a, inv)) and np.isnan(dm.msssim(ta, torch.from_numpy(inv).cuda()))
        n1, n2 = (rng.integers(0, 256, shape, dtype=np.uint8) for _ in range(2))
        got, want = dm.msssim(torch.from_numpy(n1).cuda(), torch.from_numpy(n2).cuda()), harness.calc_msssim(n1, n2)
        assert not np.isnan(want) and got == pytest.approx(want, abs=1e-12)


def test_frame_entries_match_the_host_functions(dm, golden_dir):
    """DeviceMetrics.yuv420 / rgb against harness.yuv420_distortion + yuv420_msssim / rgb_distortion on the fixtures' frames"""
    g = np.load(os.path.join(golden_dir, "frame_io_rgb.npz"))
    for name in ("f32", "f16"):
        x = torch.from_numpy(g[f"rec_c_{name}_x"]).cuda()
        rgb = torch.from_numpy(g["src_c_rgb"]).cuda()
        (p,), (s,) = dm.rgb(x, rgb, calc_ssim=True)
        assert p == pytest.approx(float(g[f"rec_c_{name}_psnr"]), abs=1e-9)
        assert s == pytest.approx(float(g[f"rec_c_{name}_msssim"]), abs=1e-12)
        assert dm.rgb(x, rgb) == ([p], [0.0])
    rng = np.random.default_rng(3)
    h, w = 180, 208
    y = _smooth_plus_noise((h, w), rng)
    u, v = _smooth_plus_noise((h // 2, w // 2), rng), _smooth_plus_noise((h // 2, w // 2), rng)
    planes = [torch.from_numpy(p).cuda() for p in (y, u, v)]
    for dtype in (torch.float16, torch.float32):
        x = harness.load_yuv420_frame(*planes, dtype)
        x = (x + torch.from_numpy(rng.normal(0, 0.02, tuple(x.shape)).astype(np.float32)).cuda().to(dtype)).contiguous()
        psnr, ms = dm.yuv420(x, *planes, calc_ssim=True)
        want_p, want_s = harness.yuv420_distortion(x, *planes), harness.yuv420_msssim(x, *planes)
        for k in range(4):
            assert psnr[k] == pytest.approx(want_p[k], abs=1e-4) and ms[k] == pytest.approx(want_s[k], abs=1e-4)
        assert psnr[1] == pytest.approx(want_p[1], abs=1e-9) and ms[1] == pytest.approx(want_s[1], abs=1e-12)    # (Y: same values)
        assert dm.yuv420(x, *planes)[1] == [0.0, 0.0, 0.0, 0.0]


# --------------------------------------------------------------------------------------------- 5. whole rate points
def _nets(mode):
    from opendcvc_amd import weights
    from opendcvc_amd.models import DMC, DMCI
    nets = []
    for cls, name in ((DMCI, "dmci"), (DMC, "dmc")):
        m = cls()
        m.load_state_dict({k: torch.from_numpy(v) for k, v in weights.make_state_dict(name, 1234).items()})
        m.to("cuda").eval()
        m.update(0.12)
        nets.append(m.half() if mode == "fp16" else m)
    return nets


@pytest.mark.parametrize("mode", ["fp32", "fp16"])
def test_png_rate_point_on_the_device_path(tmp_path, golden_dir, mode):
    """test_png_rate_point_with_msssim_matches_reference with metrics="device": same reference log, same tolerances and key
    order; against metrics="host": frame_bpp equal, the RGB planes are the same values on both paths, so PSNR within
    1e-9 dB and MS-SSIM within 1e-12"""
    sys.path.insert(0, golden_dir)
    from make_golden_png import write_png_sequence
    gold = json.load(open(os.path.join(golden_dir, "png_point.json")))
    cfg = gold["config"]
    W, H, N = cfg["width"], cfg["height"], cfg["frames"]
    src = str(tmp_path / "seq")
    write_png_sequence(src, W, H, N, cfg["src_seed"])
    i_net, p_net = _nets(mode)
    run = lambda metrics: harness.run_one_point(i_net, p_net, src, W, H, N, cfg["qp"], intra_period=cfg["intra_period"],
                                                reset_interval=cfg["reset_interval"], verbose_json=True, src_type="png",
                                                calc_ssim=True, metrics=metrics)
    got, host = run("device"), run("host")
    refs = [gold["fp32"]] + ([gold["fp16"]] if mode == "fp16" else [])
    assert list(got.keys()) == refs[0]["keys"], "log schema differs from the reference's"
    for ref in refs:
        want = ref["log"]
        assert got["frame_type"] == want["frame_type"]
        for fi in range(N):
            gb, wb = got["frame_bpp"][fi] * H * W, want["frame_bpp"][fi] * H * W
            assert abs(gb - wb) <= (8 if mode == "fp32" else 0.04 * wb + 8), (fi, gb, wb)
            assert abs(got["frame_psnr"][fi] - want["frame_psnr"][fi]) < (1e-4 if mode == "fp32" else 0.05)
            assert abs(got["frame_msssim"][fi] - want["frame_msssim"][fi]) < (1e-4 if mode == "fp32" else 5e-3)
        for k in ("ave_all_frame_bpp", "ave_all_frame_psnr", "ave_all_frame_msssim"):
            assert got[k] == pytest.approx(want[k], rel=1e-3 if mode == "fp32" else 0.02), k
    assert got["frame_bpp"] == host["frame_bpp"] and list(got.keys()) == list(host.keys())
    for fi in range(N):
        print(f"png {mode} frame {fi}: psnr diff {got['frame_psnr'][fi] - host['frame_psnr'][fi]:.3e}, "
              f"msssim diff {got['frame_msssim'][fi] - host['frame_msssim'][fi]:.3e}")
        assert abs(got["frame_psnr"][fi] - host["frame_psnr"][fi]) <= 1e-9
        assert abs(got["frame_msssim"][fi] - host["frame_msssim"][fi]) <= 1e-12


def test_yuv420_rate_point_on_the_device_path(tmp_path, golden_dir, monkeypatch):
    """test_yuv420_msssim_matches_reference with metrics="device": same reference log, tolerance and key order; against
    metrics="host": frame_bpp equal, Y PSNR within 1e-9 dB and Y MS-SSIM within 1e-12 (the same plane values on both paths).
    Chroma: the metric planes' fp32 mean ((a + b) + (d + e)) * 0.25f may differ from torch's avg_pool2d in the last bit; per
    frame, where the metric planes are torch.equal to the torch path's planes the same bounds hold for U / V, where they are
    not, U / V are bound by 1e-4 dB / 1e-4 (the tolerance the project accepts against the reference's logs).
    Measured on an MI355X (this sequence, 2 frames, 2 x 88 x 96 chroma samples each): Y planes torch.equal; 312 and 680 chroma
    samples differ from torch's avg_pool2d planes (fp32, last bit of the 2x2 sum); largest differences between the two paths:
    PSNR U 2.4e-9 dB, V 2.1e-9 dB, MS-SSIM U 5.3e-10, V 2.1e-9; Y PSNR 0, Y MS-SSIM 2.7e-15."""
    sys.path.insert(0, golden_dir)
    from make_golden_sweep import write_yuv420
    gold = json.load(open(os.path.join(golden_dir, "png_point.json")))["yuv420_msssim"]
    cfg, want = gold["config"], gold["log"]
    W, H, N = cfg["width"], cfg["height"], cfg["frames"]
    src = str(tmp_path / "seq.yuv")
    write_yuv420(src, W, H, N, cfg["src_seed"])
    i_net, p_net = _nets("fp32")
    run = lambda metrics: harness.run_one_point(i_net, p_net, src, W, H, N, cfg["qp"], intra_period=cfg["intra_period"],
                                                reset_interval=cfg["reset_interval"], verbose_json=True, calc_ssim=True,
                                                metrics=metrics)
    got = run("device")
    assert list(got.keys()) == gold["keys"]
    for k in ("frame_msssim", "frame_msssim_y", "frame_msssim_u", "frame_msssim_v", "frame_psnr"):
        for fi in range(N):
            assert abs(got[k][fi] - want[k][fi]) < 1e-4, (k, fi, got[k][fi], want[k][fi])
    assert got["ave_all_frame_msssim"] == pytest.approx(want["ave_all_frame_msssim"], abs=1e-4)
    # the host run, keeping every decoded frame to compare the two paths' chroma planes
    frames, host_fn = [], harness.yuv420_distortion
    monkeypatch.setattr(harness, "yuv420_distortion", lambda x_hat, y, u, v: frames.append(x_hat.clone()) or host_fn(x_hat, y, u, v))
    host = run("host")
    assert got["frame_bpp"] == host["frame_bpp"] and list(got.keys()) == list(host.keys()) and len(frames) == N
    dm = DeviceMetrics("cuda:0")
    for fi, x_hat in enumerate(frames):
        rec = dm.yuv420_planes(x_hat, H, W)
        y_t = torch.clamp(x_hat[:, :1, :H, :W] * 255, 0, 255)[0, 0]
        uv_t = torch.clamp(torch.nn.functional.avg_pool2d(x_hat[:, 1:, :H, :W], 2) * 255, 0, 255)[0]
        assert torch.equal(rec[0], y_t)
        differ = int((rec[1] != uv_t[0]).sum() + (rec[2] != uv_t[1]).sum())
        d = {k: abs(got[k][fi] - host[k][fi]) for k in ("frame_psnr_y", "frame_psnr_u", "frame_psnr_v", "frame_msssim_y",
                                                         "frame_msssim_u", "frame_msssim_v")}
        print(f"yuv frame {fi}: {differ} chroma samples differ from torch's planes; " + ", ".join(f"{k} {v:.3e}" for k, v in d.items()))
        assert d["frame_psnr_y"] <= 1e-9 and d["frame_msssim_y"] <= 1e-12
        for c in "uv":
            assert d[f"frame_psnr_{c}"] <= (1e-9 if differ == 0 else 1e-4)
            assert d[f"frame_msssim_{c}"] <= (1e-12 if differ == 0 else 1e-4)


# --------------------------------------------------------------------------------------------- 6. nothing but dcvc_* entries
def test_device_path_runs_no_torch_operator(dm, monkeypatch):
    """In the steady state DeviceMetrics.yuv420 / rgb dispatch no torch operator at all (so no torch kernel and no copy of a
    plane to the host: both would be operators) and call only dcvc_* entries of the library"""
    from torch.utils._python_dispatch import TorchDispatchMode
    h, w = 1080, 1920
    rng = np.random.default_rng(2)
    planes = [torch.from_numpy(rng.integers(0, 256, s, dtype=np.uint8)).cuda() for s in ((h, w), (h // 2, w // 2), (h // 2, w // 2))]
    x = harness.load_yuv420_frame(*planes, torch.float16)
    rgb = torch.from_numpy(rng.integers(0, 256, (3, 96, 128), dtype=np.uint8)).cuda()
    xr = harness.load_rgb_frame(rgb, torch.float16)
    first = dm.yuv420(x, *planes, calc_ssim=True), dm.rgb(xr, rgb, calc_ssim=True)      # (buffers are sized here)
    ops, calls = [], []

    class Recorder(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            ops.append(str(func))
            return func(*args, **(kwargs or {}))

    class CountingLib:
        def __init__(self, lib):
            self._lib = lib

        def __getattr__(self, name):
            calls.append(name)
            return getattr(self._lib, name)

    monkeypatch.setattr(dm, "_lib", CountingLib(dm._lib))
    with Recorder():
        again = dm.yuv420(x, *planes, calc_ssim=True), dm.rgb(xr, rgb, calc_ssim=True)
    assert ops == [], ops
    assert again == first                                     # (and the same input gives the same doubles)
    assert calls.count("dcvc_stream_sync") == 2 and all(c.startswith("dcvc_") for c in calls)
    assert calls.count("dcvc_frame_to_yuv420_planes") == 1 and calls.count("dcvc_frame_to_rgb") == 1
    assert calls.count("dcvc_sse") == 4 and calls.count("dcvc_msssim_stats") == 6
