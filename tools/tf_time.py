"""Developer tool: time of the temporal pre-filter's kernels (csrc/dcvc_tf.hip) on a 1080p frame - dcvc_tf_pyramid,
dcvc_tf_motion (its three launches, 4 references), dcvc_tf_blend at radius 1 (2 references) and 2 (4 references), dcvc_tf_noise
(4 references and none; in fp16 also by the number of workgroups that share its tiles, dcvc_tf_noise_workgroups) and
dcvc_tf_blend_auto beside dcvc_tf_blend at the same level, fp16 and fp32 - measured like tools/grain_time.py: warm-up, then the variants alternated batch by batch, each batch of BATCH calls
between two HIP events, medians and quartiles of the per-call time; every call works on the next of several buffer sets (more
than 512 MB of frames in all).  The frames are a smooth picture moving (2, -3) pixels per frame under noise, so the vectors
are not zero and the gathers are not aligned.  Then what the harness pays: run_one_point on a synthetic 1080p clip with the
filter off, at level 3 and at level "auto", alternated, two rounds.  Last, what "auto" chooses: a 1080p band-limited texture
moving (2, -3) per frame under noise of two strengths, coded at the fixed levels 2 .. 4 and at "auto" (synthetic weights: the
rates and PSNRs compare the configurations, they are not a codec's).
    python tools/tf_time.py [batches=100] [out=profiles/r15_tf_auto.txt] [harness frames=32, 0: kernels only] [texture frames=12, 0: none]
                             [noise workgroup sweep=1, 0: none]"""
import ctypes
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from opendcvc_amd import _lib, harness, weights

n = int(sys.argv[1]) if len(sys.argv) > 1 else 100
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                                "profiles", "r15_tf_auto.txt")
FRAMES = int(sys.argv[3]) if len(sys.argv) > 3 else 32
TEX_FRAMES = int(sys.argv[4]) if len(sys.argv) > 4 else 12
SWEEP = int(sys.argv[5]) if len(sys.argv) > 5 else 1
BATCH = 8
ACHIEVABLE = 6.3e12
H, W, Hp, Wp = 1080, 1920, 1088, 1920
L = _lib.lib()
P = lambda t: ctypes.c_void_p(t.data_ptr())
dev = torch.device("cuda", 0)
DISTS = (-1, 1, -2, 2)
BUILT_IN = L.dcvc_tf_noise_workgroups(0)         # (0 changes nothing: the count as built)


def moving_frames(dtype, seed):
    """distance -> frame: a smooth picture displaced by (2, -3) * distance, noise of 2 / 255 on each"""
    g = torch.Generator(device=dev).manual_seed(seed)
    base = torch.nn.functional.interpolate(torch.rand((1, 3, Hp // 8 + 2, Wp // 8 + 2), device=dev, generator=g), size=(Hp, Wp),
                                           mode="bicubic", align_corners=False).clamp(0, 1)
    return {d: (torch.roll(base, (2 * d, -3 * d), (2, 3)) + torch.randn((1, 3, Hp, Wp), device=dev, generator=g) * (2.0 / 255.0))
            .to(dtype).contiguous() for d in (0,) + DISTS}


def variants(dtype):
    es = torch.empty((), dtype=dtype).element_size()
    frame = 3 * Hp * Wp * es
    sets = max(2, -(-512 * 2 ** 20 // (6 * frame)))
    code = _lib.F16 if dtype == torch.float16 else _lib.F32
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    pyr_elems, gh, gw = L.dcvc_tf_pyramid_bytes(H, W) // 2, (H + 7) // 8, (W + 7) // 8
    ws = torch.empty(L.dcvc_tf_motion_ws_bytes(H, W), dtype=torch.uint8, device=dev)
    total = torch.zeros(1, dtype=torch.int64, device=dev)
    noise_ws = torch.empty(L.dcvc_tf_noise_ws_bytes(), dtype=torch.uint8, device=dev)
    result = torch.zeros(4, dtype=torch.int32, device=dev)
    totals = torch.zeros(8, dtype=torch.int64, device=dev)
    word = torch.full((1,), 3, dtype=torch.int32, device=dev)                # dcvc_tf_blend_auto's level: 3, like dcvc_tf_blend's
    data = []
    for k in range(sets):
        f = moving_frames(dtype, k)
        data.append(dict(f=f, out=torch.empty_like(f[0]), pyr=torch.empty((5, pyr_elems), dtype=torch.int16, device=dev),
                         mv=torch.empty((4, gh, gw, 2), dtype=torch.int16, device=dev),
                         err=torch.empty((4, gh, gw), dtype=torch.int32, device=dev)))
    for s in data:                               # the pyramids and vectors the timed motion / blend calls read
        for i, d in enumerate((0,) + DISTS):
            _lib.check(L.dcvc_tf_pyramid(code, P(s["f"][d]), Hp, Wp, H, W, P(s["pyr"][i]), st), "pyramid")
        s["pyrs"] = (ctypes.c_void_p * 4)(*[s["pyr"][i + 1].data_ptr() for i in range(4)])
        s["refs"] = (ctypes.c_void_p * 4)(*[s["f"][d].data_ptr() for d in DISTS])
        s["dists"] = (ctypes.c_int * 4)(*DISTS)
        _lib.check(L.dcvc_tf_motion(P(s["pyr"][0]), s["pyrs"], 4, H, W, P(s["mv"]), P(s["err"]), P(ws), st), "motion")
    torch.cuda.synchronize(dev)
    found = float(((data[0]["mv"][0, 3:-3, 3:-3].cpu() == torch.tensor([-2, 3])).all(dim=2)).float().mean())
    group = [
        ("dcvc_tf_pyramid", H * W * es + pyr_elems * 2,
         lambda k: L.dcvc_tf_pyramid(code, P(data[k]["f"][0]), Hp, Wp, H, W, P(data[k]["pyr"][0]), st)),
        ("dcvc_tf_motion 4 refs (3 launches)", 5 * pyr_elems * 2,
         lambda k: L.dcvc_tf_motion(P(data[k]["pyr"][0]), data[k]["pyrs"], 4, H, W, P(data[k]["mv"]), P(data[k]["err"]), P(ws), st)),
        ("dcvc_tf_motion 1 ref (3 launches)", 2 * pyr_elems * 2,
         lambda k: L.dcvc_tf_motion(P(data[k]["pyr"][0]), data[k]["pyrs"], 1, H, W, P(data[k]["mv"]), P(data[k]["err"]), P(ws), st)),
        ("dcvc_tf_blend radius 1 (2 refs)", 4 * frame,
         lambda k: L.dcvc_tf_blend(code, P(data[k]["f"][0]), data[k]["refs"], data[k]["dists"], 2, Hp, Wp, H, W, P(data[k]["mv"]),
                                   P(data[k]["err"]), 3, P(data[k]["out"]), P(total), st)),
        ("dcvc_tf_blend radius 2 (4 refs)", 6 * frame,
         lambda k: L.dcvc_tf_blend(code, P(data[k]["f"][0]), data[k]["refs"], data[k]["dists"], 4, Hp, Wp, H, W, P(data[k]["mv"]),
                                   P(data[k]["err"]), 3, P(data[k]["out"]), P(total), st)),
        ("dcvc_tf_blend no reference (copy)", 2 * frame,
         lambda k: L.dcvc_tf_blend(code, P(data[k]["f"][0]), data[k]["refs"], data[k]["dists"], 0, Hp, Wp, H, W, P(data[k]["mv"]),
                                   P(data[k]["err"]), 3, P(data[k]["out"]), P(total), st)),
        ("dcvc_tf_blend_auto radius 1, word 3", 4 * frame,
         lambda k: L.dcvc_tf_blend_auto(code, P(data[k]["f"][0]), data[k]["refs"], data[k]["dists"], 2, Hp, Wp, H, W, P(data[k]["mv"]),
                                        P(data[k]["err"]), P(word), P(data[k]["out"]), P(total), st)),
        ("dcvc_tf_blend_auto radius 2, word 3", 6 * frame,
         lambda k: L.dcvc_tf_blend_auto(code, P(data[k]["f"][0]), data[k]["refs"], data[k]["dists"], 4, Hp, Wp, H, W, P(data[k]["mv"]),
                                        P(data[k]["err"]), P(word), P(data[k]["out"]), P(total), st)),
        ("dcvc_tf_noise 4 refs (memset + 2)", H * W * 2 + 2 * gh * gw * 4,
         lambda k: L.dcvc_tf_noise(P(data[k]["pyr"][0]), P(data[k]["err"]), data[k]["dists"], 4, H, W, P(noise_ws), P(result),
                                   P(totals), st)),
        ("dcvc_tf_noise no reference", H * W * 2,
         lambda k: L.dcvc_tf_noise(P(data[k]["pyr"][0]), None, None, 0, H, W, P(noise_ws), P(result), P(totals), st)),
    ]
    if SWEEP and dtype == torch.float16:         # dcvc_tf_noise by the workgroups that share its tiles, in the same rotation
        for c in (64, 128, 256, 512, 1024):
            for nref in (4, 0):
                group.append((f"dcvc_tf_noise {nref} refs, {c} workgroups", H * W * 2 + (2 * gh * gw * 4 if nref else 0),
                              lambda k, c=c, nref=nref: (L.dcvc_tf_noise_workgroups(c),
                                                         L.dcvc_tf_noise(P(data[k]["pyr"][0]), P(data[k]["err"]) if nref else None,
                                                                         data[k]["dists"] if nref else None, nref, H, W, P(noise_ws),
                                                                         P(result), P(totals), st),
                                                         L.dcvc_tf_noise_workgroups(BUILT_IN))[1]))
    return group, sets, found, (data, total, noise_ws, result, totals, word)


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
    group, sets, found, keep = variants(dtype)
    L.dcvc_tf_noise(P(keep[0][0]["pyr"][0]), P(keep[0][0]["err"]), keep[0][0]["dists"], 4, H, W, P(keep[2]), P(keep[3]), None,
                    ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    lines.append(f"{tag}, {W}x{H} in a {Wp}x{Hp} tensor, {sets} buffer sets, {n} batches of {BATCH} calls per variant; "
                 f"{100 * found:.1f} % of the inner blocks of set 0 have the vector (-2, 3) of distance -1; dcvc_tf_noise of set 0 "
                 f"(noise 2 / 255): level, N, temporal, spatial = {keep[3].tolist()}")
    for (name, nbytes, _), t in zip(group, measure(group, sets)):
        q1, med, q3 = np.percentile(t, [25, 50, 75])
        rate = nbytes / (med * 1e-6)
        lines.append(f"  {name:36s} median {med:8.2f} us  quartiles {q1:8.2f} .. {q3:8.2f}  min {t.min():8.2f}  "
                     f"{nbytes / 1e6:7.2f} MB  {rate / 1e9:7.1f} GB/s = {100 * rate / ACHIEVABLE:5.1f} % of 6.3 TB/s")
    del group, keep
    torch.cuda.empty_cache()

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
            for name, kw in (("no option", {}), ("--temporal-filter 3 --tf-radius 2", dict(temporal_filter=3, tf_radius=2)),
                             ("--temporal-filter auto --tf-radius 2", dict(temporal_filter="auto", tf_radius=2)),
                             ("--temporal-filter 3 --tf-radius 1", dict(temporal_filter=3, tf_radius=1)),
                             ("--temporal-filter auto --tf-radius 1", dict(temporal_filter="auto", tf_radius=1))):
                log = harness.run_one_point(nets[0], nets[1], src, W, H, FRAMES, 32, 32, intra_period=8, verbose=1, **kw)
                rows.setdefault(name, []).append((log["avg_frame_encoding_time"] * 1e3, log["avg_frame_decoding_time"] * 1e3,
                                                  log["ave_all_frame_bpp"], log["ave_all_frame_psnr"], log.get("tf_mean_weight")))
        for name, r in rows.items():
            lines.append(f"  {name:36s} enc {r[0][0]:.3f} / {r[1][0]:.3f} ms   dec {r[0][1]:.3f} / {r[1][1]:.3f} ms   "
                         f"bpp {r[0][2]:.5f}   psnr {r[0][3]:.4f}   tf_mean_weight {r[0][4]}")

    if TEX_FRAMES:
        def texture_clip(path, sigma):
            """TEX_FRAMES frames of low-passed noise (the test texture's recipe at this size) moving (2, -3) per frame under
            Gaussian noise of sigma / 255, as 8-bit YUV 4:2:0"""
            rng = np.random.default_rng(7)
            th, tw = H + 2 * TEX_FRAMES + 8, W + 3 * TEX_FRAMES + 8
            fy, fx = np.fft.fftfreq(th)[:, None], np.fft.fftfreq(tw)[None, :]
            g = np.exp(-(fy * fy + fx * fx) / (2 * 0.06 ** 2))
            t = np.real(np.fft.ifft2(np.fft.fft2(rng.standard_normal((3, th, tw)), axes=(1, 2)) * g, axes=(1, 2)))
            lo, hi = t.min(axis=(1, 2), keepdims=True), t.max(axis=(1, 2), keepdims=True)
            t = (t - lo) / (hi - lo) * 0.9 + 0.05
            with open(path, "wb") as f:
                for i in range(TEX_FRAMES):
                    y0, x0 = 2 * i, 3 * (TEX_FRAMES - i)
                    pic = t[:, y0:y0 + H, x0:x0 + W] + rng.standard_normal((3, H, W)) * (sigma / 255.0)
                    f.write(np.clip(np.rint(pic[0] * 255.0), 0, 255).astype(np.uint8).tobytes())
                    for c in (1, 2):
                        sub = pic[c].reshape(H // 2, 2, W // 2, 2).mean(axis=(1, 3))
                        f.write(np.clip(np.rint(sub * 255.0), 0, 255).astype(np.uint8).tobytes())

        with tempfile.TemporaryDirectory() as folder:
            src = os.path.join(folder, "texture.yuv")
            lines.append(f"what auto chooses: {W} x {H} band-limited texture moving (2, -3) per frame, {TEX_FRAMES} frames, 8-bit 4:2:0, "
                         "fp16 models with the SYNTHETIC weights (rates and PSNRs compare the rows, they are no codec's), qp 32, intra "
                         "period 8, radius 2; PSNR against the UNFILTERED noisy source, as the harness reports it")
            for sigma in (1.0, 4.0):
                texture_clip(src, sigma)
                for level in (0, 2, 3, 4, "auto"):
                    log = harness.run_one_point(nets[0], nets[1], src, W, H, TEX_FRAMES, 32, 32, intra_period=8, temporal_filter=level)
                    lines.append(f"  sigma {sigma:.1f} / 255  --temporal-filter {level!s:4s}  bpp {log['ave_all_frame_bpp']:.5f}   "
                                 f"psnr {log['ave_all_frame_psnr']:.4f}   tf_mean_weight {log.get('tf_mean_weight', 0.0):.4f}"
                                 + (f"   tf_levels {log['tf_levels']}   tf_noise {log['tf_noise']:.3f}" if level == "auto" else ""))

text = "\n".join([f"csrc/dcvc_tf.hip, {torch.cuda.get_device_name(0)}; HIP events around batches of {BATCH} calls, variants "
                  "alternated batch by batch after warm-up, time per call; bytes = what the call must move once (pyramid: the "
                  "luma read + the pyramid written; motion: the pyramids read; blend: the frames read + one written; noise: Q0 and the two "
                  "error tables of distance +-1 read)"] + lines) + "\n"
print(text, end="")
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write(text)
