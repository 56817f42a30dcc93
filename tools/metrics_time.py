"""Developer tool: per-frame time of the harness's distortion metrics at 1080p 4:2:0 with an fp16 reconstruction -
metrics="host" (torch glue + numpy / scipy MS-SSIM) against metrics="device" (metrics.DeviceMetrics), alternated in one
process after warm-up; host clock around work that ends in a synchronise.  PSNR + MS-SSIM and PSNR only.
    python tools/metrics_time.py [frames=20] [out=profiles/r06_device_metrics.txt]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from opendcvc_amd import harness, weights
from opendcvc_amd.metrics import DeviceMetrics

n = int(sys.argv[1]) if len(sys.argv) > 1 else 20
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                                "profiles", "r06_device_metrics.txt")
H, W = 1080, 1920
dev = torch.device("cuda", 0)
rng = np.random.default_rng(0)
frames = []
for fi in range(4):       # a reconstruction that resembles its source, as a decoder's does
    planes = [torch.from_numpy(a).to(dev) for a in weights.synthetic_frame_yuv420(H, W, fi, 0)]
    x = harness.load_yuv420_frame(*planes, torch.float16)
    x = (x + torch.from_numpy(rng.normal(0, 0.01, tuple(x.shape)).astype(np.float32)).to(dev).half()).contiguous()
    frames.append((x, planes))
dm = DeviceMetrics(dev)


def host(x, planes, ssim):
    p = harness.yuv420_distortion(x, *planes)
    return p, (harness.yuv420_msssim(x, *planes) if ssim else [0.0] * 4)


def device(x, planes, ssim):
    return dm.yuv420(x, *planes, ssim)


def timed(fn, x, planes, ssim):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    r = fn(x, planes, ssim)
    torch.cuda.synchronize(dev)
    return time.perf_counter() - t0, r


lines = []
for ssim in (True, False):
    for fn in (host, device):
        timed(fn, *frames[0], ssim)                                      # warm-up: buffers, code objects, scipy plans
    t = {"host": [], "device": []}
    worst = 0.0
    for k in range(n):
        x, planes = frames[k % len(frames)]
        th, rh = timed(host, x, planes, ssim)
        td, rd = timed(device, x, planes, ssim)
        t["host"].append(th)
        t["device"].append(td)
        worst = max(worst, max(abs(a - b) for a, b in zip(rh[0] + rh[1], rd[0] + rd[1])))
    what = "PSNR + MS-SSIM" if ssim else "PSNR only"
    for name in ("host", "device"):
        a = np.asarray(t[name]) * 1e3
        lines.append(f"{what:15s} metrics={name:6s}: median {np.median(a):9.3f} ms  min {a.min():9.3f}  max {a.max():9.3f}  "
                     f"mean {a.mean():9.3f}  ({n} frames)")
    lines.append(f"{what:15s} host / device (medians): {np.median(t['host']) / np.median(t['device']):.1f} x; "
                 f"largest |host - device| over the logged values: {worst:.3e}")
text = "\n".join([f"1080p YUV 4:2:0, fp16 reconstruction, {torch.cuda.get_device_name(0)}; per-frame metric time, host clock "
                  "around synchronised work, host and device alternated frame by frame"] + lines) + "\n"
print(text, end="")
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write(text)
