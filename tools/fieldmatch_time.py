"""Developer tool: what the deinterlacer's film mode (docs/deinterlace.md, "Film mode") costs on one MI355X, fp16.
1. dcvc_field_match (with a previous frame), dcvc_field_weave behind a word that reads 0 and behind one that reads 1, between two
   HIP events at 1080p and 2160p, operands rotated call by call through buffer sets of more than 512 MB, the variants alternated
   call by call after warm-up; each against its floor at 6.3 TB/s - the luma of two frames read once; nothing; half a frame read
   and written - and against a launch with nothing to do (a weave of a 4 x 8 picture behind a word that reads 0).
2. Deinterlacer("film").filter(): wall time per call on an idle stream, the launches only (nothing is waited for).
3. The harness on a telecined 1920 x 1080 clip: run_one_point's avg_frame_encoding_time / avg_frame_decoding_time (the frames
   behind the first ten) with --deinterlace off, film + --frame-dup, on and off again (the second 'off' shows the spread),
   alternated round by round in one process.
    python tools/fieldmatch_time.py [rounds=5] [out=profiles/r23_field_match.txt] [harness-only | off-only]
off-only: three points with the option off behind a warm-up point, their times and the sha256 of each container - for a
comparison of two trees, a fresh process each."""
import ctypes
import hashlib
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from opendcvc_amd import _lib, harness, weights

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                                "profiles", "r23_field_match.txt")
only = sys.argv[3] if len(sys.argv) > 3 else ""
CALLS = 300
STREAM_TBS = 6.3               # what a streaming kernel reaches here (README)
dev = torch.device("cuda", 0)
torch.set_grad_enabled(False)
torch.set_num_threads(1)
L = _lib.lib()
lines = [f"film mode, {torch.cuda.get_device_name(0)}, fp16"]
P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
pad = lambda n: n + (-n) % 16


# ---------------------------------------------------------------------------------- 1. the kernels, 2. the object
def kernel_times(H, W):
    from opendcvc_amd.deinterlace import Deinterlacer
    Hp, Wp = pad(H), pad(W)
    n = 3 * Hp * Wp
    sets = -(-512 * 2 ** 20 // (2 * n)) + 2
    fr = [torch.rand(n, dtype=torch.float16, device=dev).view(1, 3, Hp, Wp) for _ in range(sets)]
    words = torch.tensor([0, 1], dtype=torch.int32, device=dev)
    word = lambda k: ctypes.c_void_p(words.data_ptr() + 4 * k)
    need = L.dcvc_field_match_ws_bytes()
    ws = torch.zeros(need + 8, dtype=torch.uint8, device=dev)
    verdict = ctypes.c_void_p(ws.data_ptr() + need)

    def weave(k, w, hp=Hp, wp=Wp, h=H, ww=W):
        return L.dcvc_field_weave(_lib.F16, P(fr[k % sets]), hp, wp, h, ww, 0, 2, word(w), P(fr[(k + 1) % sets]), stream())

    plane = H * W * 2
    variants = [("field_match, prev", 2 * plane, lambda k: L.dcvc_field_match(_lib.F16, P(fr[k % sets]), P(fr[(k + 1) % sets]), Hp, Wp, H, W,
                                                                              0, P(ws), verdict, stream())),
                ("field_match, no prev", plane, lambda k: L.dcvc_field_match(_lib.F16, P(fr[k % sets]), None, Hp, Wp, H, W, 0, P(ws),
                                                                             verdict, stream())),
                ("field_weave, word 0", 0, lambda k: weave(k, 0)),
                ("field_weave, word 1", 3 * plane, lambda k: weave(k, 1)),             # half of three planes read, half written
                ("weave of 4 x 8, word 0", 0, lambda k: weave(k, 0, 16, 16, 4, 8))]     # a 16 x 16 frame: an empty launch between two events
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
    assert not ws.cpu().numpy()[:16].any()
    lines.append(f"{W} x {H}: HIP events around each launch, {CALLS} calls per entry, alternated call by call; operands rotated "
                 f"through {sets} sets ({sets * n * 2 / 2 ** 20:.0f} MB); 4:2:0 chroma lines; uniform noise: every candidate is combed")
    for (label, nbytes, _), e in zip(variants, ev):
        t = np.asarray([a.elapsed_time(b) * 1e3 for a, b in e])
        q1, med, q3 = np.percentile(t, [25, 50, 75])
        line = f"  {label:24s} {nbytes / 1e6:7.2f} MB  median {med:7.2f} us  quartiles {q1:7.2f} .. {q3:7.2f}  min {t.min():7.2f}"
        if nbytes:
            floor = nbytes / (STREAM_TBS * 1e12) * 1e6
            line += f"  floor {floor:6.2f} us  x{med / floor:6.1f}  {nbytes / (med * 1e-6) / 1e12:5.2f} TB/s"
        lines.append(line)

    di = Deinterlacer(dev, "film", "tff", 2)
    for k in range(32):
        di.filter(fr[k % sets], (H, W))
    torch.cuda.synchronize(dev)
    t = []
    for k in range(CALLS):
        t0 = time.perf_counter()
        di.filter(fr[k % sets], (H, W))
        t.append((time.perf_counter() - t0) * 1e6)
        if k % 16 == 15:
            torch.cuda.synchronize(dev)
    q1, med, q3 = np.percentile(t, [25, 50, 75])
    lines.append(f"  Deinterlacer('film').filter(): host time per call (the output's allocation and three launches; nothing is "
                 f"waited for)  median {med:7.2f} us  quartiles {q1:7.2f} .. {q3:7.2f}  min {min(t):7.2f}")
    del di, variants, fr
    torch.cuda.empty_cache()


if not only:
    kernel_times(1080, 1920)
    kernel_times(2160, 3840)

# ---------------------------------------------------------------------------------- 3. the harness
H, W, FRAMES = 1080, 1920, 30
nets = harness.load_nets(None, None, 0.12, False, "cuda:0")
tri = lambda k: k % 14 if k % 14 < 8 else 14 - k % 14            # forth and back: the generator's shift never wraps
with tempfile.TemporaryDirectory() as d:
    content = [weights.synthetic_frame_yuv420(H, W, k, 0) for k in range(8)]
    src = os.path.join(d, "telecined.yuv")
    with open(src, "wb") as f:
        for k in range(FRAMES):                                   # 3:2 pulldown: film pictures A A|B B|C C D, cycle of five frames
            c, r = divmod(k, 5)
            first, second = content[tri(4 * c + (0, 0, 1, 2, 3)[r])], content[tri(4 * c + (0, 1, 2, 2, 3)[r])]
            for a, b in zip(first, second):
                plane = np.array(a)
                plane[1::2] = b[1::2]
                f.write(plane.tobytes())

    def point(kw, bin_path=None):
        log = harness.run_one_point(*nets, src, W, H, FRAMES, 32, 32, verbose=1, bin_path=bin_path, **kw)
        return (log["avg_frame_encoding_time"] * 1e3, log["avg_frame_decoding_time"] * 1e3, log["ave_all_frame_bpp"],
                log.get("field_matches"), log.get("deint_frames"), log.get("repeat_frames"))

    if only == "off-only":
        point({})
        for k in range(3):
            path = os.path.join(d, "off.bin")
            enc, dec, bpp = point({}, path)[:3]
            print(f"off point {k}: encode {enc:.3f} decode {dec:.3f} ms per frame  bpp {bpp:.5f}  sha256 "
                  f"{hashlib.sha256(open(path, 'rb').read()).hexdigest()}")
        sys.exit(0)

    VARIANTS = [("off", {}), ("film", {"deinterlace": "film", "frame_dup": True}), ("on", {"deinterlace": "on"}), ("off2", {})]
    for _, kw in VARIANTS[:3]:
        point(kw)                                                 # warm-up
    res = {tag: [] for tag, _ in VARIANTS}
    for _ in range(rounds):
        for tag, kw in VARIANTS:
            res[tag].append(point(kw))
    lines.append(f"harness, {W} x {H}, {FRAMES} telecined frames (3:2 pulldown; 1 I + P, qp 32, fp16): avg_frame_encoding_time / "
                 f"avg_frame_decoding_time over the frames behind the first ten, {rounds} rounds alternated in one process after "
                 f"warm-up; off2 = off once more (the spread); film = film + frame_dup: field_matches {res['film'][0][3]}, filtered "
                 f"{res['film'][0][4]}, repeats {res['film'][0][5]}; bpp off {res['off'][0][2]:.4f} film {res['film'][0][2]:.4f} on "
                 f"{res['on'][0][2]:.4f} (random-weight nets: the bpp says nothing about a trained model)")
    for col, what in ((0, "encode"), (1, "decode")):
        med = {}
        for tag, _ in VARIANTS:
            t = np.asarray([r[col] for r in res[tag]])
            med[tag] = float(np.median(t))
            lines.append(f"  {what} {tag:4s} median {med[tag]:7.3f}  min {t.min():7.3f}  max {t.max():7.3f}  ms per frame")
        lines.append(f"  {what} film - off: {(med['film'] - med['off']) * 1e3:+.1f} us   on - off: {(med['on'] - med['off']) * 1e3:+.1f} us   "
                     f"off2 - off: {(med['off2'] - med['off']) * 1e3:+.1f} us per frame")
text = "\n".join(lines) + "\n"
print(text, end="")
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write(text)
