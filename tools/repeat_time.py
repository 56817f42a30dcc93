"""Developer tool: what repeated-frame coding (docs/frame_repeat.md) costs and saves on one MI355X, fp16.
1. dcvc_frame_maxdiff between two HIP events at 1080p and 2160p, from 16-byte-aligned frames (the 16-byte form) and from frames
   one element off (the narrow form), operands rotated call by call through buffer sets of more than 512 MB, the variants
   alternated call by call after warm-up; each against its traffic floor - both frames once at 6.3 TB/s - and against a
   16 x 16 compare between the same events (the floor of one launch).
2. RepeatDetector.is_repeat() on frames that are no repeats: wall time per call, the wait for the compare's event included -
   what every frame that is coded pays.
3. The harness on 1920 x 1080: run_one_point's avg_frame_encoding_time / avg_frame_decoding_time (the frames behind the first
   ten) and bpp on a clip whose every second frame repeats the one before, and on a clip without repeats, with --frame-dup
   off, on and off again (the second 'off' shows the spread), alternated round by round in one process.
    python tools/repeat_time.py [rounds=5] [out=profiles/r21_frame_repeat.txt] [harness-only]"""
import ctypes
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from opendcvc_amd import _lib, harness, weights
from opendcvc_amd.entropy import PinnedBuffer
from opendcvc_amd.repeat import RepeatDetector

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                                "profiles", "r21_frame_repeat.txt")
harness_only = len(sys.argv) > 3 and sys.argv[3] == "harness-only"
CALLS = 300
STREAM_TBS = 6.3               # what a streaming kernel reaches here (README)
dev = torch.device("cuda", 0)
torch.set_grad_enabled(False)
torch.set_num_threads(1)
L = _lib.lib()
lines = [f"repeated-frame coding, {torch.cuda.get_device_name(0)}, fp16"]
P = lambda t: ctypes.c_void_p(t.data_ptr())
stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
pad = lambda n: n + (-n) % 16


# ---------------------------------------------------------------------------------- 1. the kernel, 2. the detector
def kernel_times(H, W):
    Hp, Wp = pad(H), pad(W)
    n = 3 * Hp * Wp
    sets = -(-512 * 2 ** 20 // (2 * n)) + 1
    flat = [torch.rand(n + 16, dtype=torch.float16, device=dev) for _ in range(sets)]
    wide = [f[:n].view(1, 3, Hp, Wp) for f in flat]               # 16-byte aligned: the 16-byte form
    off = [f[1:n + 1].view(1, 3, Hp, Wp) for f in flat]           # one element on: the narrow form
    assert wide[0].data_ptr() % 16 == 0 and off[0].data_ptr() % 16 == 2
    ws = torch.zeros(L.dcvc_frame_maxdiff_ws_bytes(), dtype=torch.uint8, device=dev)
    pinned = PinnedBuffer(16)
    out = ctypes.c_void_p(pinned.ptr)
    call = lambda fr, k, h, w: L.dcvc_frame_maxdiff(_lib.F16, P(fr[k % sets]), P(fr[(k + 1) % sets]), Hp, Wp, h, w, P(ws), out, stream())
    variants = [("16-byte form", 2 * 3 * H * W * 2, lambda k: call(wide, k, H, W)),
                ("narrow form", 2 * 3 * H * W * 2, lambda k: call(off, k, H, W)),
                ("compare of 16 x 16", 0, lambda k: call(wide, k, 16, 16))]          # the floor of one launch between two events
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
    assert not ws.cpu().numpy().any()
    lines.append(f"{W} x {H}: dcvc_frame_maxdiff, HIP events around each launch, {CALLS} calls per entry, alternated call by call; "
                 f"operands rotated through {sets} sets ({sets * n * 2 / 2 ** 20:.0f} MB)")
    for (label, nbytes, _), e in zip(variants, ev):
        t = np.asarray([a.elapsed_time(b) * 1e3 for a, b in e])
        q1, med, q3 = np.percentile(t, [25, 50, 75])
        line = f"  {label:18s} {nbytes / 1e6:7.2f} MB  median {med:7.2f} us  quartiles {q1:7.2f} .. {q3:7.2f}  min {t.min():7.2f}"
        if nbytes:
            floor = nbytes / (STREAM_TBS * 1e12) * 1e6
            line += f"  floor {floor:6.2f} us  x{med / floor:6.1f}  {nbytes / (med * 1e-6) / 1e12:5.2f} TB/s"
        lines.append(line)

    det = RepeatDetector(dev, 0.0)
    for k in range(32):
        det.is_repeat(wide[k % sets], (H, W))
    torch.cuda.synchronize(dev)
    t = []
    for k in range(CALLS):
        t0 = time.perf_counter()
        rep = det.is_repeat(wide[k % sets], (H, W))
        t.append((time.perf_counter() - t0) * 1e6)
        assert not rep
    q1, med, q3 = np.percentile(t, [25, 50, 75])
    lines.append(f"  is_repeat() on frames that are no repeats, an idle stream: wall time per call, the wait included  "
                 f"median {med:7.2f} us  quartiles {q1:7.2f} .. {q3:7.2f}  min {min(t):7.2f}")
    del variants, flat, wide, off, det
    torch.cuda.empty_cache()


if not harness_only:
    kernel_times(1080, 1920)
    kernel_times(2160, 3840)

# ---------------------------------------------------------------------------------- 3. the harness
H, W, FRAMES = 1080, 1920, 30
nets = harness.load_nets(None, None, 0.12, False, "cuda:0")
tri = lambda k: k % 14 if k % 14 < 8 else 14 - k % 14            # forth and back: the generator's shift never wraps
with tempfile.TemporaryDirectory() as d:
    content = [weights.synthetic_frame_yuv420(H, W, k, 0) for k in range(8)]
    clips = {}
    for name, index in (("every second frame a repeat", lambda k: tri(k // 2)), ("no repeats", tri)):
        clips[name] = os.path.join(d, f"{len(clips)}.yuv")
        with open(clips[name], "wb") as f:
            for k in range(FRAMES):
                for plane in content[index(k)]:
                    f.write(plane.tobytes())

    def point(src, dup):
        kw = {"frame_dup": True} if dup else {}
        log = harness.run_one_point(*nets, src, W, H, FRAMES, 32, 32, verbose=1, **kw)
        return (log["avg_frame_encoding_time"] * 1e3, log["avg_frame_decoding_time"] * 1e3, log["ave_all_frame_bpp"],
                log.get("repeat_frames"))

    VARIANTS = [("off", False), ("on", True), ("off2", False)]
    for name, src in clips.items():
        for _, dup in VARIANTS[:2]:
            point(src, dup)                                       # warm-up
        res = {tag: [] for tag, _ in VARIANTS}
        for _ in range(rounds):
            for tag, dup in VARIANTS:
                res[tag].append(point(src, dup))
        lines.append(f"harness, {W} x {H}, {FRAMES} frames, {name} (1 I + P, qp 32, fp16): avg_frame_encoding_time / "
                     f"avg_frame_decoding_time over the frames behind the first ten, {rounds} rounds alternated in one process "
                     f"after warm-up; off2 = off once more (the spread); on found {res['on'][0][3]} repeats, bpp "
                     f"{res['on'][0][2]:.4f} against {res['off'][0][2]:.4f}")
        for col, what in ((0, "encode"), (1, "decode")):
            med = {}
            for tag, _ in VARIANTS:
                t = np.asarray([r[col] for r in res[tag]])
                med[tag] = float(np.median(t))
                lines.append(f"  {what} {tag:4s} median {med[tag]:7.3f}  min {t.min():7.3f}  max {t.max():7.3f}  ms per frame")
            lines.append(f"  {what} on / off: {med['on'] / med['off']:.3f}   off2 / off: {med['off2'] / med['off']:.3f}   "
                         f"on - off: {(med['on'] - med['off']) * 1e3:+.1f} us per frame")
text = "\n".join(lines) + "\n"
print(text, end="")
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write(text)
