"""`python bench.py --gpus 1 --steps K --warmup W` as the driver runs it: a plain run times the K steps and prints the
headline line only (the sequential GOP and the roofline / exact-mode / CPU legs are behind --full), and --dump-outputs
writes what the last timed step computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_times_the_steps_and_dumps_the_last_one(tmp_path):
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "LOCAL_WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    out_dir = tmp_path / "dump"
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5",
                        "--dump-outputs", str(out_dir)], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [json.loads(ln) for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    out = lines[0]
    assert out["steps"] == 20 and out["warmup"] == 5 and out["n_gpus"] == 1
    assert out["unit"] == "frames/s" and out["higher_is_better"] is True and out["dtype"] == "f16"
    assert out["value"] > 0 and out["ms_per_step"] == pytest.approx(1e3 / out["value"], rel=2e-3)
    for key in ("vs_baseline", "enc_fps_per_gpu", "psnr", "reference_gop", "roofline", "exact_mode", "cpu_baseline"):
        assert key not in out, key
    assert out["config"]["full"] is False

    names = sorted(os.listdir(out_dir))
    assert names == ["bit_stream.npy", "packet.npy", "x_hat.npy"]
    assert sum(os.path.getsize(os.path.join(out_dir, n)) for n in names) <= 64 * 2 ** 20
    got = {n[:-4]: np.load(os.path.join(out_dir, n)) for n in names}
    assert all(a.dtype == np.float32 for a in got.values())
    is_i, qp, use_ada_i, nbytes = got["packet"]
    assert is_i in (0, 1) and use_ada_i in (0, 1) and 0 <= qp < 64
    assert got["bit_stream"].shape == (int(nbytes),) and nbytes > 0
    assert np.array_equal(got["bit_stream"], np.round(got["bit_stream"])) and got["bit_stream"].max() <= 255
    assert got["x_hat"].shape == (1, 3, 1088, 1920) and np.isfinite(got["x_hat"]).all()
