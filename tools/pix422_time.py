"""Developer tool: time of the 4:2:2 frame I/O kernels (csrc/dcvc_pix422.hip) at 1920 x 1080 and 3840 x 2160 with an fp16
model - uyvy422, v210 and yuv422p10le - with the yuv444p10le and yuv420p10le loader / storer of csrc/dcvc_pixfmt.hip as the
yardstick, in one process and one rotation: warm-up, then the variants alternated launch by launch, each launch between two
HIP events; medians and quartiles over the launches, and operand bytes (the file's frame + the model frame's padded area or
picture) over the median.  Every launch works on the next of several buffer sets (more than 512 MB in all) so that no
operand is still in a cache.  Then one harness run per format at 1920 x 1080 (synthetic weights, 14 frames, the first 10
warm-up as in the harness's own clocks): ms per encoded and per decoded frame against a yuv444p10le run of the same picture.
    python tools/pix422_time.py [launches=200] [out=profiles/r25_pix422.txt] [harness=1]"""
import ctypes
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from opendcvc_amd import _lib, harness, weights
from opendcvc_amd.pipeline import PixelFormat
from opendcvc_amd.pix422 import Format422

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
n = int(sys.argv[1]) if len(sys.argv) > 1 else 200
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "r25_pix422.txt")
with_harness = int(sys.argv[3]) if len(sys.argv) > 3 else 1
ACHIEVABLE = 6.3e12
dev = torch.device("cuda", 0)
L = _lib.lib()
P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def variants(H, W):
    """-> {"load": [(name, bytes, launch(k))], "store": [...]}, number of buffer sets"""
    pb, pr = (-H) % 16, (-W) % 16
    Hp, Wp = H + pb, W + pr
    sets = max(2, -(-512 * 2 ** 20 // (3 * Hp * Wp * 2)))
    frames = [torch.rand((1, 3, Hp, Wp), device=dev).half() for _ in range(sets)]      # the storers' input
    outs = [torch.empty((1, 3, Hp, Wp), dtype=torch.float16, device=dev) for _ in range(sets)]
    load, store = [], []
    for name in ("yuv444p10le", "yuv420p10le"):
        f = PixelFormat.parse(name)
        shapes = f.plane_shapes(H, W)
        src = [[torch.randint(0, 1024, s, dtype=torch.int32, device=dev).to(torch.int16) for s in shapes] for _ in range(sets)]
        dst = [[torch.empty_like(p) for p in src[0]] for _ in range(sets)]
        ys, cs = shapes[0][1], shapes[1][1]
        args = (_lib.F16, f.chroma, f.bit_depth, 0, 0)
        load.append((f"dcvc_planes_to_frame {name}", f.frame_bytes(H, W) + 3 * Hp * Wp * 2,
                     lambda k, src=src, args=args, ys=ys, cs=cs: L.dcvc_planes_to_frame(
                         *args, P(src[k][0]), P(src[k][1]), P(src[k][2]), ys, cs, H, W, pb, pr, P(outs[k]), stream())))
        store.append((f"dcvc_frame_to_planes {name}", f.frame_bytes(H, W) + 3 * H * W * 2,
                      lambda k, dst=dst, args=args, ys=ys, cs=cs: L.dcvc_frame_to_planes(
                          *args, P(frames[k]), Hp, Wp, H, W, P(dst[k][0]), P(dst[k][1]), P(dst[k][2]), ys, cs, stream())))
    for name in ("uyvy422", "v210", "yuv422p10le"):
        f = Format422.parse(name)
        if f.packed:
            # (any bytes are a picture; bits 30 and 31 of a v210 word are not read)
            src = [[torch.randint(0, 256, s, dtype=torch.int32, device=dev).to(torch.uint8) for s in f.plane_shapes(H, W)] + [None, None]
                   for _ in range(sets)]
            ys, cs = f.row_bytes(W), 0
        else:
            src = [[torch.randint(0, 1024, s, dtype=torch.int32, device=dev).to(torch.int16) for s in f.plane_shapes(H, W)]
                   for _ in range(sets)]
            ys, cs = W, W // 2
        dst = [[torch.empty_like(p) if p is not None else None for p in src[0]] for _ in range(sets)]
        args = (_lib.F16, f.layout, f.bit_depth)
        load.append((f"dcvc_yuv422_to_frame {name}", f.frame_bytes(H, W) + 3 * Hp * Wp * 2,
                     lambda k, src=src, args=args, ys=ys, cs=cs: L.dcvc_yuv422_to_frame(
                         *args, P(src[k][0]), P(src[k][1]), P(src[k][2]), ys, cs, H, W, pb, pr, P(outs[k]), stream())))
        store.append((f"dcvc_frame_to_yuv422 {name}", f.frame_bytes(H, W) + 3 * H * W * 2,
                      lambda k, dst=dst, args=args, ys=ys, cs=cs: L.dcvc_frame_to_yuv422(
                          *args, P(frames[k]), Hp, Wp, H, W, P(dst[k][0]), P(dst[k][1]), P(dst[k][2]), ys, cs, stream())))
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


def harness_lines():
    """one run per format of the same 1920 x 1080 picture (the 4:2:2 samples of a synthetic clip; the 4:4:4 file doubles the
    chroma columns)"""
    H, W, N = 1080, 1920, 14
    nets = harness.load_nets(None, None, 0.12, False, dev)
    clip = []
    for i in range(N):
        y, u, v = weights.synthetic_frame_yuv420(H, W, i, 3)
        clip.append([p.astype(np.uint16) << 2 for p in (y, np.repeat(u, 2, axis=0), np.repeat(v, 2, axis=0))])

    def v210(y, u, v):
        g = (W + 5) // 6
        Y, Cb, Cr = (np.zeros((H, g * k), np.uint32) for k in (6, 3, 3))
        Y[:, :W], Cb[:, :W // 2], Cr[:, :W // 2] = y, u, v
        Y, Cb, Cr = Y.reshape(H, g, 6), Cb.reshape(H, g, 3), Cr.reshape(H, g, 3)
        words = np.zeros((H, Format422.parse("v210").row_bytes(W) // 4), "<u4")
        q = words[:, :4 * g].reshape(H, g, 4)
        q[..., 0] = Cb[..., 0] | Y[..., 0] << 10 | Cr[..., 0] << 20
        q[..., 1] = Y[..., 1] | Cb[..., 1] << 10 | Y[..., 2] << 20
        q[..., 2] = Cr[..., 1] | Y[..., 3] << 10 | Cb[..., 2] << 20
        q[..., 3] = Y[..., 4] | Cr[..., 2] << 10 | Y[..., 5] << 20
        return [words]

    def uyvy(y, u, v):
        s = np.zeros((H, W // 2, 4), np.uint8)
        s[..., 0], s[..., 1], s[..., 2], s[..., 3] = u >> 2, y[:, 0::2] >> 2, v >> 2, y[:, 1::2] >> 2
        return [s]

    files = {"yuv444p10le": lambda y, u, v: [y, np.repeat(u, 2, axis=1), np.repeat(v, 2, axis=1)],
             "yuv422p10le": lambda y, u, v: [y, u, v], "v210": v210, "uyvy422": uyvy}
    out = [f"harness, {W} x {H}, fp16, {N} frames (the first 10 warm-up), qp 32, --metrics device --save_decoded_frame: ms per frame"]
    with tempfile.TemporaryDirectory() as tmp:
        for name, make in files.items():
            path = os.path.join(tmp, name + ".raw")
            with open(path, "wb") as fp:
                for planes in clip:
                    for p in make(*planes):
                        fp.write(np.ascontiguousarray(p).tobytes())
            log = harness.run_one_point(nets[0], nets[1], path, W, H, N, 32, 32, src_type=name, metrics="device", verbose=1,
                                        rec_path=os.path.join(tmp, name + ".rec"))
            out.append(f"  {name:12s} encode {1e3 * log['avg_frame_encoding_time']:8.3f} ms  decode {1e3 * log['avg_frame_decoding_time']:8.3f} ms"
                       f"  bpp {log['ave_all_frame_bpp']:.4f}")
    return out


lines = []
for H, W in ((1080, 1920), (2160, 3840)):
    groups, sets = variants(H, W)
    lines.append(f"{W} x {H}, fp16 model, {sets} buffer sets, {n} launches per variant")
    for kind in ("load", "store"):
        times = measure(groups[kind], sets)
        for (name, nbytes, _), t in zip(groups[kind], times):
            q1, med, q3 = np.percentile(t, [25, 50, 75])
            rate = nbytes / (med * 1e-6)
            lines.append(f"  {kind:5s} {name:36s} median {med:8.2f} us  quartiles {q1:8.2f} .. {q3:8.2f}  min {t.min():8.2f}  "
                         f"{nbytes / 1e6:7.2f} MB  {rate / 1e12:5.2f} TB/s = {100 * rate / ACHIEVABLE:5.1f} % of 6.3 TB/s")
    del groups
    torch.cuda.empty_cache()
if with_harness:
    lines += harness_lines()
text = "\n".join([f"4:2:2 frame I/O kernels, {torch.cuda.get_device_name(0)}; HIP events around single launches, variants alternated launch "
                  "by launch after warm-up; bytes = the file's frame + the model frame (loaders: the padded frame written; storers: "
                  "the picture read)"] + lines) + "\n"
print(text, end="")
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write(text)
