"""Developer tool: what active-area coding (docs/active_area.md) costs and saves on one MI355X, fp16.
1. dcvc_bars_scan, dcvc_bars_extent, dcvc_frame_window and dcvc_frame_paste between two HIP events at 1080p (138-row bars) and
   2160p (276-row bars), operands rotated call by call through buffer sets of more than 512 MB each, the variants alternated
   call by call after warm-up; each time against its traffic floor: the bytes it must move at 6.3 TB/s.
2. The harness on 1920 x 1080 with 138-row bars: run_one_point's avg_frame_encoding_time / avg_frame_decoding_time (the frames
   behind the first ten) with crop off, auto and off again (the second 'off' shows the spread), alternated round by round in
   one process.
    python tools/bars_time.py [rounds=5] [out=profiles/r20_active_area.txt] [harness-only]"""
import ctypes
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from opendcvc_amd import _lib, harness, weights
from opendcvc_amd.entropy import PinnedBuffer

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                                "profiles", "r20_active_area.txt")
harness_only = len(sys.argv) > 3 and sys.argv[3] == "harness-only"
CALLS = 300
STREAM_TBS = 6.3               # what a streaming kernel reaches here (README)
dev = torch.device("cuda", 0)
torch.set_grad_enabled(False)
torch.set_num_threads(1)
L = _lib.lib()
lines = [f"active-area coding, {torch.cuda.get_device_name(0)}, fp16"]
P = lambda t: ctypes.c_void_p(t.data_ptr())
stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
pad = lambda n: n + (-n) % 16


# ---------------------------------------------------------------------------------- 1. the kernels
def kernel_times(H, W, bar):
    Hp, Wp, HO = pad(H), pad(W), H - 2 * bar
    HOp = pad(HO)
    full_bytes, win_bytes = 3 * Hp * Wp * 2, 3 * HOp * Wp * 2
    sets = -(-512 * 2 ** 20 // full_bytes) + 1
    full = [torch.rand((1, 3, Hp, Wp), dtype=torch.float16, device=dev) for _ in range(sets)]
    for x in full:
        x[:, :, :bar] = 0.0625
        x[:, :, H - bar:] = 0.0625
    wins = [torch.rand((1, 3, HOp, Wp), dtype=torch.float16, device=dev) for _ in range(sets)]
    outs_full = [torch.empty_like(full[0]) for _ in range(sets)]
    outs_win = [torch.empty_like(wins[0]) for _ in range(sets)]
    ws = torch.empty(L.dcvc_bars_ws_bytes(H, W), dtype=torch.uint8, device=dev)
    ws_small = torch.empty(L.dcvc_bars_ws_bytes(16, 16), dtype=torch.uint8, device=dev)
    pinned = PinnedBuffer(32)
    colour = (ctypes.c_float * 3)(0.0625, 0.5, 0.5)
    _lib.check(L.dcvc_bars_reset(P(ws), H, W, stream()), "dcvc_bars_reset")
    variants = [
        ("dcvc_bars_scan", 3 * H * W * 2,
         lambda k: L.dcvc_bars_scan(_lib.F16, P(full[k % sets]), Hp, Wp, H, W, P(ws), stream())),
        ("scan of 16 x 16", 3 * 16 * 16 * 2,          # the floor of one launch between two events
         lambda k: L.dcvc_bars_scan(_lib.F16, P(full[k % sets]), Hp, Wp, 16, 16, P(ws_small), stream())),
        ("dcvc_bars_extent", 24 * (H + W),
         lambda k: L.dcvc_bars_extent(P(ws), H, W, 0.0, ctypes.c_void_p(pinned.ptr), stream())),
        ("dcvc_frame_window", 3 * HO * W * 2 + win_bytes,
         lambda k: L.dcvc_frame_window(_lib.F16, P(full[k % sets]), Hp, Wp, H, W, bar, 0, P(outs_win[k % sets]), HOp, Wp, HO, W,
                                       stream())),
        ("dcvc_frame_paste", 3 * HO * W * 2 + full_bytes,
         lambda k: L.dcvc_frame_paste(_lib.F16, P(wins[k % sets]), HOp, Wp, HO, W, P(outs_full[k % sets]), Hp, Wp, H, W, bar, 0,
                                      colour, stream())),
    ]
    for _, _, fn in variants:
        for k in range(min(sets, 16)):
            _lib.check(fn(k), "warm-up")
    torch.cuda.synchronize(dev)
    ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(CALLS)] for _ in variants]
    for k in range(CALLS):
        for vi, v in enumerate(variants):
            a, b = ev[vi][k]
            a.record()
            rc = v[2](k)
            b.record()
            _lib.check(rc, v[0])
        if k % 16 == 15:
            torch.cuda.synchronize(dev)
    torch.cuda.synchronize(dev)
    found = np.array(pinned.view(np.int32, 8))
    lines.append(f"{W} x {H} with {bar}-row bars (window {W} x {HO}): HIP events around each launch, {CALLS} calls per entry, "
                 f"alternated call by call; operands rotated through {sets} sets ({sets * full_bytes / 2 ** 20:.0f} MB); "
                 f"extents read {found[:5].tolist()}")
    for (label, nbytes, _), e in zip(variants, ev):
        t = np.asarray([a.elapsed_time(b) * 1e3 for a, b in e])
        q1, med, q3 = np.percentile(t, [25, 50, 75])
        floor = nbytes / (STREAM_TBS * 1e12) * 1e6
        line = f"  {label:18s} {nbytes / 1e6:7.2f} MB  median {med:7.2f} us  quartiles {q1:7.2f} .. {q3:7.2f}  min {t.min():7.2f}"
        if floor >= 0.1:                                          # (an entry that moves next to nothing has no traffic floor)
            line += f"  floor {floor:6.2f} us  x{med / floor:6.1f}  {nbytes / (med * 1e-6) / 1e12:5.2f} TB/s"
        lines.append(line)
    del variants, full, wins, outs_full, outs_win
    torch.cuda.empty_cache()


if not harness_only:
    kernel_times(1080, 1920, 138)
    kernel_times(2160, 3840, 276)

# ---------------------------------------------------------------------------------- 2. the harness
H, W, BAR, FRAMES = 1080, 1920, 138, 30
nets = harness.load_nets(None, None, 0.12, False, "cuda:0")
tri = lambda k: k % 14 if k % 14 < 8 else 14 - k % 14            # forth and back: the generator's shift never wraps
with tempfile.TemporaryDirectory() as d:
    src = os.path.join(d, "barred.yuv")
    content = [weights.synthetic_frame_yuv420(H - 2 * BAR, W, k, 0) for k in range(8)]
    with open(src, "wb") as f:
        for k in range(FRAMES):
            for i, plane in enumerate(content[tri(k)]):
                b = BAR if i == 0 else BAR // 2
                full = np.full((plane.shape[0] + 2 * b, plane.shape[1]), 16 if i == 0 else 128, np.uint8)
                full[b:b + plane.shape[0]] = plane
                f.write(full.tobytes())

    def point(crop):
        kw = {"crop": crop} if crop else {}
        log = harness.run_one_point(*nets, src, W, H, FRAMES, 32, 32, verbose=1, **kw)
        return log["avg_frame_encoding_time"] * 1e3, log["avg_frame_decoding_time"] * 1e3, log.get("active_area"), log["ave_all_frame_bpp"]

    VARIANTS = [("off", None), ("auto", "auto"), ("off2", None)]
    for _, crop in VARIANTS[:2]:
        point(crop)                                               # warm-up: graph captures at both sizes
    res = {tag: [] for tag, _ in VARIANTS}
    for _ in range(rounds):
        for tag, crop in VARIANTS:
            res[tag].append(point(crop))
lines.append(f"harness, {W} x {H} with {BAR}-row bars, {FRAMES} frames (1 I + P, qp 32, fp16): avg_frame_encoding_time / "
             f"avg_frame_decoding_time over the frames behind the first ten, {rounds} rounds alternated in one process after "
             f"warm-up; off2 = off once more (the spread); auto found {res['auto'][0][2]}, bpp {res['auto'][0][3]:.4f} against "
             f"{res['off'][0][3]:.4f}")
for col, what in ((0, "encode"), (1, "decode")):
    med = {}
    for tag, _ in VARIANTS:
        t = np.asarray([r[col] for r in res[tag]])
        med[tag] = float(np.median(t))
        lines.append(f"  {what} {tag:4s} median {med[tag]:7.3f}  min {t.min():7.3f}  max {t.max():7.3f}  ms per frame")
    lines.append(f"  {what} auto / off: {med['auto'] / med['off']:.3f}   off2 / off: {med['off2'] / med['off']:.3f}   "
                 f"(pixel ratio {(H - 2 * BAR) / H:.3f})")
text = "\n".join(lines) + "\n"
print(text, end="")
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write(text)
