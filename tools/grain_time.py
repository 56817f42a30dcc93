"""Developer tool: time of the film-grain kernels (csrc/dcvc_grain.hip) on a 1080p frame - dcvc_grain_apply for corr 0, 1, 2 and
dcvc_grain_stats, fp16 and fp32 - measured like tools/resize_time.py: warm-up, then the variants alternated batch by batch,
each batch of BATCH launches between two HIP events, medians and quartiles of the per-launch time, bytes over the median
against the 6.3 TB/s a streaming kernel can reach on an MI355X; every launch works on the next of several buffer sets (more
than 512 MB in all).  Then what the harness pays: the host's wall time of FilmGrain.apply + synchronize (every decoded
frame while a unit is in force) and of FilmGrain.estimate (every I frame of an "auto" encode), and run_one_point on a
synthetic 1080p clip with film_grain None / fixed / "auto", alternated, two rounds.
    python tools/grain_time.py [batches=100] [out=profiles/r13_film_grain.txt] [harness frames=32, 0: kernels only]"""
import ctypes
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from opendcvc_amd import _lib, harness, weights
from opendcvc_amd.grain import FilmGrain, GrainParams, _c_params

n = int(sys.argv[1]) if len(sys.argv) > 1 else 100
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                                "profiles", "r13_film_grain.txt")
FRAMES = int(sys.argv[3]) if len(sys.argv) > 3 else 32
BATCH = 8
ACHIEVABLE = 6.3e12
H, W, Hp, Wp = 1080, 1920, 1088, 1920
L = _lib.lib()
P = lambda t: ctypes.c_void_p(t.data_ptr())
dev = torch.device("cuda", 0)
PARAMS = [GrainParams(7, corr, (20, 24, 28, 32, 36, 40, 44, 48), 16, 12) for corr in (0, 1, 2)]


def variants(dtype):
    es = torch.empty((), dtype=dtype).element_size()
    nbytes = 2 * 3 * Hp * Wp * es                                  # the frame read once and written once
    sets = max(2, -(-512 * 2 ** 20 // nbytes))
    frames = [torch.rand((1, 3, Hp, Wp), device=dev).to(dtype) for _ in range(sets)]
    outs = [torch.empty_like(f) for f in frames]
    table = torch.zeros((12, 2), dtype=torch.int64, device=dev)
    code = _lib.F16 if dtype == torch.float16 else _lib.F32
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    group = []
    for p in PARAMS:
        cp = _c_params(p)
        calls = [(code, P(frames[k]), Hp, Wp, H, W, P(outs[k]), cp, 3, st) for k in range(sets)]
        group.append((f"dcvc_grain_apply corr {p.corr}", nbytes, lambda k, calls=calls: L.dcvc_grain_apply(*calls[k])))
    calls = [(code, P(frames[k]), P(frames[(k + 1) % sets]), Hp, Wp, H, W, P(table), st) for k in range(sets)]
    group.append(("dcvc_grain_stats", nbytes, lambda k, calls=calls: L.dcvc_grain_stats(*calls[k])))
    return group, sets


def measure(group, sets):
    for _, _, launch in group:
        for k in range(sets):
            launch(k)
    torch.cuda.synchronize(dev)
    events = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)] for _ in group]
    k = 0
    for it in range(n):
        for vi, (_, _, launch) in enumerate(group):
            a, b = events[vi][it]
            a.record()
            for _ in range(BATCH):
                rc = launch(k % sets)
                k += 1
            b.record()
            _lib.check(rc, "launch")
        if it % 16 == 15:
            torch.cuda.synchronize(dev)
    torch.cuda.synchronize(dev)
    return [np.asarray([a.elapsed_time(b) * 1e3 / BATCH for a, b in ev]) for ev in events]


lines = []
for dtype, tag in ((torch.float16, "fp16"), (torch.float32, "fp32")):
    group, sets = variants(dtype)
    lines.append(f"{tag}, {W}x{H} in a {Wp}x{Hp} tensor, {sets} buffer sets, {n} batches of {BATCH} launches per variant")
    for (name, nbytes, _), t in zip(group, measure(group, sets)):
        q1, med, q3 = np.percentile(t, [25, 50, 75])
        rate = nbytes / (med * 1e-6)
        lines.append(f"  {name:26s} median {med:8.2f} us  quartiles {q1:8.2f} .. {q3:8.2f}  min {t.min():8.2f}  "
                     f"{nbytes / 1e6:7.2f} MB  {rate / 1e9:7.1f} GB/s = {100 * rate / ACHIEVABLE:5.1f} % of 6.3 TB/s")
    del group
    torch.cuda.empty_cache()

# the host's side of one call, fp16: wall time from the call to the end of a synchronisation, against the synchronisation alone
fg = FilmGrain(dev)
x = torch.rand((1, 3, Hp, Wp), device=dev).half()
y = torch.rand((1, 3, Hp, Wp), device=dev).half()
out = torch.empty_like(x)


def wall(fn, reps=200):
    for _ in range(10):
        fn()
    torch.cuda.synchronize(dev)
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(dev)
        t.append((time.perf_counter() - t0) * 1e6)
    return np.percentile(t, [25, 50, 75])


lines.append("host wall time of one call + torch.cuda.synchronize, fp16 1080p, 200 calls (quartiles, us)")
for name, fn in (("synchronize alone", lambda: None),
                 ("FilmGrain.apply corr 2 (every decoded frame under a unit)", lambda: fg.apply(x, (H, W), PARAMS[2], 3, out=out)),
                 ("FilmGrain.estimate (every I frame of an auto encode: launch, read-back, host)", lambda: fg.estimate(x, y, (H, W), 0))):
    q1, med, q3 = wall(fn)
    lines.append(f"  {name:82s} {q1:8.1f} {med:8.1f} {q3:8.1f}")

if FRAMES:
    from opendcvc_amd.models import DMC, DMCI
    nets = []
    for cls, name in ((DMCI, "dmci"), (DMC, "dmc")):
        m = cls()
        m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in weights.make_state_dict(name, 1234).items()})
        m.to(dev).eval()
        m.update(0.12)
        nets.append(m.half())
    with tempfile.TemporaryDirectory() as folder:
        src = os.path.join(folder, "clip.yuv")
        with open(src, "wb") as f:
            for i in range(FRAMES):
                for plane in weights.synthetic_frame_yuv420(H, W, i % 8, 3):
                    f.write(plane.tobytes())
        lines.append(f"harness, {W} x {H} synthetic clip, {FRAMES} frames, fp16 models, qp 32, intra period 8, host entropy coder; the "
                     "harness's own avg_frame_encoding_time / avg_frame_decoding_time (frames 11 .. , device synchronised per frame), "
                     "one process, the configurations alternated, two rounds")
        rows = {}
        for rnd in range(2):
            for name, fgopt in (("no option", None), ("fixed GrainParams corr 2", PARAMS[2]), ("auto", "auto")):
                log = harness.run_one_point(nets[0], nets[1], src, W, H, FRAMES, 32, 32, intra_period=8, verbose=1,
                                            film_grain=fgopt)
                rows.setdefault(name, []).append((log["avg_frame_encoding_time"] * 1e3, log["avg_frame_decoding_time"] * 1e3,
                                                  log["ave_all_frame_bpp"], log["ave_all_frame_psnr"], log.get("grain_units")))
        for name, r in rows.items():
            lines.append(f"  {name:28s} enc {r[0][0]:.3f} / {r[1][0]:.3f} ms   dec {r[0][1]:.3f} / {r[1][1]:.3f} ms   "
                         f"bpp {r[0][2]:.5f}   psnr {r[0][3]:.4f}   grain units {r[0][4]}")

text = "\n".join([f"csrc/dcvc_grain.hip, {torch.cuda.get_device_name(0)}; HIP events around batches of {BATCH} launches, variants "
                  "alternated batch by batch after warm-up, time per launch; bytes = the padded frame read once + written once "
                  "(stats: two frames read)"] + lines) + "\n"
print(text, end="")
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write(text)
