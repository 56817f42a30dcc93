"""The device-side distortion path (csrc/dcvc_metrics.hip, opendcvc_amd/metrics.py) as far as a GPU-less host can check
it: the new entries are declared, bound and exported, `--metrics` reaches the worker pool's options and run_one_point, and
the host-side end of MS-SSIM (the product over the per-level means) agrees with harness.calc_msssim."""
import ctypes
import os
import re

import numpy as np
import pytest

from opendcvc_amd import _lib, harness

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dcvc_frame_to_yuv420_planes", "dcvc_sse", "dcvc_msssim_ws_bytes", "dcvc_msssim_stats")


def test_metric_entries_are_declared_bound_and_exported():
    header = open(os.path.join(REPO, "include", "dcvc_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert os.path.exists(_lib.LIB_PATH), "libdcvc_amd.so not built (run __graft_entry__.build())"
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, code), f"{name} not declared in dcvc_amd.h"
        assert name in _lib.EXPORTS and hasattr(L, name), name
    assert re.search(r"\bDCVC_U8\s*=\s*2\b", code) and _lib.U8 == 2
    assert re.search(r"#define\s+DCVC_SSE_BLOCKS\s+%d\b" % _lib.SSE_BLOCKS, header)
    lib = _lib.lib()                                      # (argument checks run without a device)
    assert lib.dcvc_msssim_ws_bytes(87, 200) < 0 and lib.dcvc_msssim_ws_bytes(200, 87) < 0
    # 1080p: the fp64 planes of scales 1 - 4 (two planes each) and two partial sums per 32 x 16 tile of every scale
    sizes = [(1080, 1920), (540, 960), (270, 480), (135, 240), (68, 120)]
    want = 8 * (2 * sum(h * w for h, w in sizes[1:]) + 2 * sum(-(-(h - 10) // 16) * -(-(w - 10) // 32) for h, w in sizes))
    assert lib.dcvc_msssim_ws_bytes(1080, 1920) == want


def test_metrics_option_parses_and_reaches_the_pool_options(monkeypatch):
    for k in ("HIP_VISIBLE_DEVICES", "ROCR_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setattr(harness, "count_gpus", lambda: 1)
    ap = harness.build_parser()
    for argv, want in (("--test_config m.json", "host"), ("--test-config m.json --metrics host", "host"),
                       ("--test_config m.json --metrics device --calc_ssim 1", "device"),
                       ("--test-config m.json --metrics=device --calc-ssim", "device")):
        args = ap.parse_args(argv.split())
        assert args.metrics == want
        assert harness.manifest_options(args, ap)[0]["metrics"] == want
    assert ap.parse_args("--src a.yuv --width 64 --height 64 --frames 1".split()).metrics == "host"
    with pytest.raises(SystemExit):
        ap.parse_args("--test_config m.json --metrics gpu".split())


def test_run_job_hands_the_option_to_run_one_point(monkeypatch):
    seen = []
    monkeypatch.setattr(harness, "run_one_point", lambda *a, **kw: seen.append(kw["metrics"]) or {})
    job = dict(ds_name="S", seq="s.yuv", src_path="s.yuv", src_width=64, src_height=64, frame_num=1, qp_i=0, qp_p=0,
               intra_period=-1, reset_interval=32)
    harness.run_job(("i", "p"), job, {})
    harness.run_job(("i", "p"), job, dict(metrics="host"))
    harness.run_job(("i", "p"), job, dict(metrics="device"))
    assert seen == ["host", "host", "device"]


def test_unknown_metrics_value_is_refused_before_any_device_work():
    with pytest.raises(ValueError, match="bogus"):
        harness.run_one_point(None, None, "/nonexistent.yuv", 64, 64, 1, 0, metrics="bogus")


def test_msssim_from_level_means_is_the_hosts_last_line():
    """metrics.msssim_from_stats on the per-level means the host path forms == harness.calc_msssim, NaN included"""
    from scipy import ndimage
    from opendcvc_amd.metrics import msssim_from_stats
    rng = np.random.default_rng(5)
    for shape in ((96, 130), (180, 200)):
        a = rng.integers(0, 256, shape).astype(np.float64)
        for b in (np.clip(a + rng.normal(0, 6.0, shape), 0, 255), 255 - a):
            ssim, cs, x, y = [], [], a, b
            for _ in range(5 if min(shape) >= 176 else 4):
                s_map, c_map = harness._ssim_and_cs(x, y, harness._gauss_window(), 255)
                ssim.append(s_map.mean())
                cs.append(c_map.mean())
                x = ndimage.convolve(x, np.full((2, 2), 0.25), mode="reflect")[::2, ::2]
                y = ndimage.convolve(y, np.full((2, 2), 0.25), mode="reflect")[::2, ::2]
            got, want = msssim_from_stats(ssim, cs), harness.calc_msssim(a, b)
            assert (np.isnan(got) and np.isnan(want)) or got == want
    assert np.isnan(harness.calc_msssim(a, 255 - a))
