"""Developer tool: time of the temporal pre-filter's quarter-pel kernels (csrc/dcvc_tf_subpel.hip) on a 1080p fp16 frame -
dcvc_tf_refine and dcvc_tf_blend_subpel at radius 1 (2 references) and 2 (4 references), subpel 1 and 2, on material that moves
(0.75, -1.25) pixels per frame (nearly every block ends fractional) and on static material (nearly none does), beside the same
run's dcvc_tf_motion, dcvc_tf_blend and dcvc_tf_blend_auto - measured like tools/tf_time.py: warm-up, then the variants
alternated batch by batch, each batch of BATCH calls between two HIP events, medians and quartiles of the per-call time; every
call works on the next of several buffer sets.  With a second library (parent=...: the build of another commit) its
dcvc_tf_motion, dcvc_tf_refine and three blend entries run in the same rotation.  Then what the harness pays: run_one_point on a synthetic 1080p
clip with the filter off, at level 3, and at level 3 with --tf-subpel 0 / 1 / 2, alternated, two rounds; root=DIR measures the
package of another checkout instead (its rows with --tf-subpel are left out where it has no such option).
    python tools/tf_subpel_time.py [batches=100] [out=profiles/r16_tf_subpel.txt] [frames=32, 0: kernels only] [kernels=1]
                                   [parent=LIB] [root=DIR] [append=1: add to the file]"""
import ctypes
import os
import sys
import tempfile

args = dict(a.split("=", 1) for a in sys.argv[1:])
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOT = os.path.abspath(args.get("root", HERE))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from opendcvc_amd import _lib, harness, weights

n = int(args.get("batches", 100))
out_path = args.get("out", os.path.join(HERE, "profiles", "r16_tf_subpel.txt"))
FRAMES = int(args.get("frames", 32))
KERNELS = int(args.get("kernels", 1))
BATCH = 8
ACHIEVABLE = 6.3e12
H, W, Hp, Wp = 1080, 1920, 1088, 1920
L = _lib.lib()
P = lambda t: ctypes.c_void_p(t.data_ptr())
dev = torch.device("cuda", 0)
DISTS = (-1, 1, -2, 2)
MATERIALS = {"moving (0.75, -1.25)": (0.75, -1.25), "static": (0.0, 0.0)}


def frames_of(per_frame, seed):
    """distance -> fp16 frame: a smooth picture displaced by per_frame * distance (a Fourier phase ramp: fractions included),
    noise of 2 / 255 on each"""
    g = torch.Generator(device=dev).manual_seed(seed)
    base = torch.nn.functional.interpolate(torch.rand((1, 3, Hp // 8 + 2, Wp // 8 + 2), device=dev, generator=g), size=(Hp, Wp),
                                           mode="bicubic", align_corners=False).clamp(0, 1)
    spec = torch.fft.fft2(base)
    fy, fx = torch.fft.fftfreq(Hp, device=dev)[:, None], torch.fft.fftfreq(Wp, device=dev)[None, :]
    out = {}
    for d in (0,) + DISTS:
        moved = torch.fft.ifft2(spec * torch.exp(-2j * np.pi * (fy * per_frame[0] * d + fx * per_frame[1] * d))).real
        out[d] = (moved + torch.randn((1, 3, Hp, Wp), device=dev, generator=g) * (2.0 / 255.0)).to(torch.float16).contiguous()
    return out


def variants(parent):
    es, code = 2, _lib.F16
    frame = 3 * Hp * Wp * es
    sets = max(2, -(-256 * 2 ** 20 // (6 * frame)))
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    pyr_elems, gh, gw = L.dcvc_tf_pyramid_bytes(H, W) // 2, (H + 7) // 8, (W + 7) // 8
    ws = torch.empty(L.dcvc_tf_motion_ws_bytes(H, W), dtype=torch.uint8, device=dev)
    total = torch.zeros(1, dtype=torch.int64, device=dev)
    word = torch.full((1,), 3, dtype=torch.int32, device=dev)
    group, notes, keep = [], [], [ws, total, word]
    for mi, (name, per_frame) in enumerate(MATERIALS.items()):
        data = []
        for k in range(sets):
            f = frames_of(per_frame, 100 * mi + k)
            s = dict(f=f, out=torch.empty_like(f[0]), pyr=torch.empty((5, pyr_elems), dtype=torch.int16, device=dev),
                     mv=torch.empty((4, gh, gw, 2), dtype=torch.int16, device=dev), err=torch.empty((4, gh, gw), dtype=torch.int32, device=dev),
                     mvq=torch.empty((4, gh, gw, 2), dtype=torch.int16, device=dev), errq=torch.empty((4, gh, gw), dtype=torch.int32, device=dev))
            for i, d in enumerate((0,) + DISTS):
                _lib.check(L.dcvc_tf_pyramid(code, P(f[d]), Hp, Wp, H, W, P(s["pyr"][i]), st), "pyramid")
            s["pyrs"] = (ctypes.c_void_p * 4)(*[s["pyr"][i + 1].data_ptr() for i in range(4)])
            s["refs"] = (ctypes.c_void_p * 4)(*[f[d].data_ptr() for d in DISTS])
            s["dists"] = (ctypes.c_int * 4)(*DISTS)
            _lib.check(L.dcvc_tf_motion(P(s["pyr"][0]), s["pyrs"], 4, H, W, P(s["mv"]), P(s["err"]), P(ws), st), "motion")
            for sp in (1, 2):                    # the refined vectors the timed blends read
                s[f"mvq{sp}"], s[f"errq{sp}"] = torch.empty_like(s["mv"]), torch.empty_like(s["err"])
                _lib.check(L.dcvc_tf_refine(P(s["pyr"][0]), s["pyrs"], 4, H, W, sp, P(s["mv"]), P(s["err"]), P(s[f"mvq{sp}"]),
                                            P(s[f"errq{sp}"]), st), "refine")
            data.append(s)
        torch.cuda.synchronize(dev)
        keep.append(data)
        frac = [float((data[0][f"mvq{sp}"] & 3).ne(0).any(dim=3).float().mean()) for sp in (1, 2)]
        zero = float(data[0]["err"].eq(0).float().mean())
        notes.append(f"{name}: {100 * frac[0]:.1f} % / {100 * frac[1]:.1f} % of the vectors fractional at subpel 1 / 2, "
                     f"{100 * zero:.1f} % of the blocks with a level-0 SAD of 0")

        def add(label, nbytes, call, data=data):
            group.append((f"{label}, {name.split()[0]}", nbytes, lambda k: call(data[k])))
        libs = [("", L)] + ([(" (parent)", parent)] if parent is not None else [])
        for nref in (2, 4):
            radius = nref // 2
            for tag, lib in libs:
                add(f"dcvc_tf_motion {nref} refs (3 launches){tag}", (1 + nref) * pyr_elems * 2,
                    lambda s, nref=nref, lib=lib: lib.dcvc_tf_motion(P(s["pyr"][0]), s["pyrs"], nref, H, W, P(s["mv"]), P(s["err"]), P(ws), st))
                for sp in (1, 2):
                    add(f"dcvc_tf_refine {nref} refs subpel {sp}{tag}", (1 + nref) * H * W * 2,
                        lambda s, nref=nref, sp=sp, lib=lib: lib.dcvc_tf_refine(P(s["pyr"][0]), s["pyrs"], nref, H, W, sp, P(s["mv"]),
                                                                                P(s["err"]), P(s["mvq"]), P(s["errq"]), st))
            for tag, lib in libs:
                add(f"dcvc_tf_blend radius {radius}{tag}", (2 + nref) * frame,
                    lambda s, nref=nref, lib=lib: lib.dcvc_tf_blend(code, P(s["f"][0]), s["refs"], s["dists"], nref, Hp, Wp, H, W, P(s["mv"]),
                                                                    P(s["err"]), 3, P(s["out"]), P(total), st))
                add(f"dcvc_tf_blend_auto radius {radius}{tag}", (2 + nref) * frame,
                    lambda s, nref=nref, lib=lib: lib.dcvc_tf_blend_auto(code, P(s["f"][0]), s["refs"], s["dists"], nref, Hp, Wp, H, W,
                                                                         P(s["mv"]), P(s["err"]), P(word), P(s["out"]), P(total), st))
                for sp in (1, 2):
                    add(f"dcvc_tf_blend_subpel radius {radius} subpel {sp}{tag}", (2 + nref) * frame,
                        lambda s, nref=nref, sp=sp, lib=lib: lib.dcvc_tf_blend_subpel(code, P(s["f"][0]), s["refs"], s["dists"], nref, Hp, Wp,
                                                                                      H, W, P(s[f"mvq{sp}"]), P(s[f"errq{sp}"]), 3, None,
                                                                                      P(s["out"]), P(total), st))
    return group, sets, notes, keep


def measure(group, sets):
    for _, _, launch in group:
        for k in range(sets):
            _lib.check(launch(k), "launch")
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
if KERNELS:
    parent = None
    if "parent" in args:
        parent = ctypes.CDLL(os.path.abspath(args["parent"]))
        for name in ("dcvc_tf_blend", "dcvc_tf_blend_auto", "dcvc_tf_blend_subpel", "dcvc_tf_refine", "dcvc_tf_motion"):
            getattr(parent, name).restype, getattr(parent, name).argtypes = getattr(L, name).restype, getattr(L, name).argtypes
    group, sets, notes, keep = variants(parent)
    lines.append(f"fp16, {W}x{H} in a {Wp}x{Hp} tensor, {sets} buffer sets per material, {n} batches of {BATCH} calls per variant, level 3; "
                 "bytes = what the call must move once (motion: the pyramids read; refine: the Q0 planes read; blend: the frames "
                 "read + one written - the blend's traffic floor is bytes / 6.3 TB/s)" + ("; (parent): the other library's entry" if parent else ""))
    lines += ["  " + s for s in notes]
    for (name, nbytes, _), t in zip(group, measure(group, sets)):
        q1, med, q3 = np.percentile(t, [25, 50, 75])
        lines.append(f"  {name:61s} median {med:8.2f} us  quartiles {q1:8.2f} .. {q3:8.2f}  min {t.min():8.2f}  "
                     f"{nbytes / 1e6:7.2f} MB  floor {nbytes / ACHIEVABLE * 1e6:6.2f} us")
    del group, keep
    torch.cuda.empty_cache()

if FRAMES:
    import inspect
    from opendcvc_amd.models import DMC, DMCI
    nets = []
    for cls, name in ((DMCI, "dmci"), (DMC, "dmc")):
        m = cls()
        m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in weights.make_state_dict(name, 1234).items()})
        m.to(dev).eval()
        m.update(0.12)
        nets.append(m.half())
    has_option = "tf_subpel" in inspect.signature(harness.run_one_point).parameters
    configs = [("no option", {}), ("--temporal-filter 3", dict(temporal_filter=3))]
    if has_option:
        configs += [(f"--temporal-filter 3 --tf-subpel {sp}", dict(temporal_filter=3, tf_subpel=sp)) for sp in (0, 2, 1)]
    with tempfile.TemporaryDirectory() as folder:
        src = os.path.join(folder, "clip.yuv")
        with open(src, "wb") as f:
            for i in range(FRAMES):
                for plane in weights.synthetic_frame_yuv420(H, W, i % 8, 3):
                    f.write(plane.tobytes())
        lines.append(f"harness of {os.path.relpath(ROOT, HERE) if ROOT != HERE else 'this tree'}, {W} x {H} synthetic clip, {FRAMES} frames, "
                     "fp16 models, qp 32, intra period 8, radius 2, host entropy coder; the harness's own avg_frame_encoding_time (frames "
                     "11 .. , device synchronised per frame), one process, the configurations alternated, two rounds")
        rows = {}
        for rnd in range(2):
            for name, kw in configs:
                log = harness.run_one_point(nets[0], nets[1], src, W, H, FRAMES, 32, 32, intra_period=8, verbose=1, **kw)
                rows.setdefault(name, []).append((log["avg_frame_encoding_time"] * 1e3, log["ave_all_frame_bpp"], log["ave_all_frame_psnr"],
                                                  log.get("tf_mean_weight")))
        for name, r in rows.items():
            lines.append(f"  {name:36s} enc {r[0][0]:.3f} / {r[1][0]:.3f} ms   bpp {r[0][1]:.5f}   psnr {r[0][2]:.4f}   tf_mean_weight {r[0][3]}")

text = "\n".join([f"csrc/dcvc_tf_subpel.hip beside csrc/dcvc_tf.hip, {torch.cuda.get_device_name(0)}; HIP events around batches of {BATCH} "
                  "calls, variants alternated batch by batch after warm-up, time per call"] + lines) + "\n"
print(text, end="")
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "a" if args.get("append") else "w") as f:
    f.write(text)
