"""Developer tool: time of the frame I/O kernels at 1920 x 1080 and 3840 x 2160 with an fp16 model - the 8-bit planar
4:2:0 kernels (dcvc_yuv420_to_frame / dcvc_frame_to_yuv420) against the loader / storer of csrc/dcvc_pixfmt.hip for
yuv420p10le, yuv444p10le, nv12 and p010le, in one process: warm-up, then the variants alternated launch by launch, each
launch between two HIP events; medians and quartiles over the launches, and operand bytes (planes + the model frame's
picture or padded area) over the median against the 6.3 TB/s a streaming kernel can reach on an MI355X.  Every launch
works on the next of several buffer sets (more than 512 MB in all) so that no operand is still in a cache.
    python tools/pixfmt_time.py [launches=200] [out=profiles/r07_pixfmt_io.txt]"""
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from opendcvc_amd import _lib
from opendcvc_amd.pipeline import PixelFormat

n = int(sys.argv[1]) if len(sys.argv) > 1 else 200
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                                "profiles", "r07_pixfmt_io.txt")
ACHIEVABLE = 6.3e12
dev = torch.device("cuda", 0)
L = _lib.lib()
P = lambda t: ctypes.c_void_p(t.data_ptr())
stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
FORMATS = ["yuv420p10le", "yuv444p10le", "nv12", "p010le"]


def samples(shape, fmt):
    """random samples of the format on the device (16-bit words as an int16 view: the kernels only see the pointer)"""
    v = torch.randint(0, fmt.max_val + 1, shape, dtype=torch.int32, device=dev) << (16 - fmt.bit_depth if fmt.msb_aligned else 0)
    return v.to(torch.uint8) if fmt.sample_bytes == 1 else v.to(torch.int16)


def variants(H, W):
    """-> {"load": [(name, bytes, launch(k))], "store": [...]}, number of buffer sets"""
    pb, pr = (-H) % 16, (-W) % 16
    Hp, Wp = H + pb, W + pr
    sets = max(2, -(-512 * 2 ** 20 // (3 * Hp * Wp * 2)))
    frames = [torch.rand((1, 3, Hp, Wp), device=dev).half() for _ in range(sets)]      # the storers' input
    outs = [torch.empty((1, 3, Hp, Wp), dtype=torch.float16, device=dev) for _ in range(sets)]
    f8 = PixelFormat("yuv420p", 420, 8)
    p8 = [[samples(s, f8) for s in f8.plane_shapes(H, W)] for _ in range(sets)]
    q8 = [[torch.empty_like(p) for p in p8[0]] for _ in range(sets)]
    load = [("dcvc_yuv420_to_frame (8-bit planar 4:2:0)", f8.frame_bytes(H, W) + 3 * Hp * Wp * 2,
             lambda k: L.dcvc_yuv420_to_frame(_lib.F16, P(p8[k][0]), P(p8[k][1]), P(p8[k][2]), H, W, pb, pr, P(outs[k]), stream()))]
    store = [("dcvc_frame_to_yuv420 (8-bit planar 4:2:0)", f8.frame_bytes(H, W) + 3 * H * W * 2,
              lambda k: L.dcvc_frame_to_yuv420(_lib.F16, P(frames[k]), Hp, Wp, H, W, 0, P(q8[k][0]), P(q8[k][1]), P(q8[k][2]), stream()))]
    for name in FORMATS:
        f = PixelFormat.parse(name)
        shapes = f.plane_shapes(H, W)
        src = [[samples(s, f) for s in shapes] for _ in range(sets)]
        dst = [[torch.empty_like(p) for p in src[0]] for _ in range(sets)]
        ys, cs = shapes[0][1], shapes[1][1]
        third = lambda planes: P(planes[2]) if len(planes) == 3 else None
        args = (_lib.F16, f.chroma, f.bit_depth, int(f.semi_planar), int(f.msb_aligned))
        load.append((f"dcvc_planes_to_frame {name}", f.frame_bytes(H, W) + 3 * Hp * Wp * 2,
                     lambda k, src=src, args=args, ys=ys, cs=cs: L.dcvc_planes_to_frame(
                         *args, P(src[k][0]), P(src[k][1]), third(src[k]), ys, cs, H, W, pb, pr, P(outs[k]), stream())))
        store.append((f"dcvc_frame_to_planes {name}", f.frame_bytes(H, W) + 3 * H * W * 2,
                      lambda k, dst=dst, args=args, ys=ys, cs=cs: L.dcvc_frame_to_planes(
                          *args, P(frames[k]), Hp, Wp, H, W, P(dst[k][0]), P(dst[k][1]), third(dst[k]), ys, cs, stream())))
    return {"load": load, "store": store}, sets


def measure(group, sets):
    for _, _, launch in group:                                     # warm-up: code objects, every buffer set touched once
        for k in range(sets):
            _lib.check(launch(k), "warm-up")
    torch.cuda.synchronize(dev)
    events = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)] for _ in group]
    for it in range(n):
        for vi, (_, _, launch) in enumerate(group):
            a, b = events[vi][it]
            a.record()
            rc = launch((it * len(group) + vi) % sets)
            b.record()
            _lib.check(rc, "launch")
        if it % 16 == 15:
            torch.cuda.synchronize(dev)                            # (keeps the queue of events short)
    torch.cuda.synchronize(dev)
    return [np.asarray([a.elapsed_time(b) * 1e3 for a, b in ev]) for ev in events]      # microseconds


lines = []
for H, W in ((1080, 1920), (2160, 3840)):
    groups, sets = variants(H, W)
    lines.append(f"{W} x {H}, fp16 model, {sets} buffer sets, {n} launches per variant")
    for kind in ("load", "store"):
        times = measure(groups[kind], sets)
        stats = []
        for (name, nbytes, _), t in zip(groups[kind], times):
            q1, med, q3 = np.percentile(t, [25, 50, 75])
            stats.append((q1, med, q3))
            rate = nbytes / (med * 1e-6)
            lines.append(f"  {kind:5s} {name:44s} median {med:8.2f} us  quartiles {q1:8.2f} .. {q3:8.2f}  min {t.min():8.2f}  "
                         f"{nbytes / 1e6:7.2f} MB  {rate / 1e12:5.2f} TB/s = {100 * rate / ACHIEVABLE:5.1f} % of 6.3 TB/s")
        (pq1, pmed, pq3), (nq1, nmed, nq3) = stats[0], stats[1]
        spread = max(pq3 - pq1, nq3 - nq1)
        verdict = "not slower" if nmed <= pmed + spread else "SLOWER"
        lines.append(f"  {kind:5s} yuv420p10le against the 8-bit kernel: {nmed:.2f} us against {pmed:.2f} us, quartile spread {spread:.2f} us: "
                     f"{verdict} ({pmed / nmed:.2f} x)")
    del groups
    torch.cuda.empty_cache()
text = "\n".join([f"frame I/O kernels, {torch.cuda.get_device_name(0)}; HIP events around single launches, variants alternated launch by "
                  "launch after warm-up; bytes = the planes + the model frame (loaders: the padded frame written; storers: the picture read)"]
                 + lines) + "\n"
print(text, end="")
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write(text)
