"""Developer tool: what the frame lookahead costs on one MI355X (docs/lookahead.md).
1. dcvc_lookahead_cost (three launches) between two HIP events at the plane sizes of 1080p (135 x 240) and 4K (270 x 480),
   operands alternated call by call over plane pairs of more than 512 MB in all, against the same pair over and over and
   against the 1 x 1 plane of an 8 x 8 picture (three launches with nothing to do: the floor); the variants alternate call by
   call after warm-up.  Then Lookahead.words() from the host's side: enqueue and the one synchronisation.
2. The harness at 1080p fp16 on material without a cut: avg_frame_encoding_time of run_one_point with scenecut 150 and
   lookahead 4 against scenecut 150 alone, each in a fresh child process, alternated round by round (the order rotates).
3. With a second source tree (the parent commit, built): scenecut 150 without the option in this tree against that tree, the
   same way.
    python tools/lookahead_time.py [rounds=3] [out=profiles/r17_lookahead.txt] [parent tree]
   Both tables twice: with the interpreter's garbage collector as it is, and switched off for the timed run (a full
   collection costs milliseconds, and whether one lands among the 32 timed frames depends on the allocations since start).
    python tools/lookahead_time.py point <tree> <yuv> <frames> <lookahead> <collector 0 | 1>        (what the children run)"""
import ctypes
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, FRAMES, QP = 1080, 1920, 42, 32


def point(tree, yuv, frames, lookahead, collector):
    sys.path.insert(0, tree)
    import gc
    import torch
    from opendcvc_amd import harness
    torch.set_grad_enabled(False)
    torch.set_num_threads(1)
    nets = harness.load_nets(None, None, 0.12, False, "cuda:0")
    kw = dict(intra_period=-1, reset_interval=32, verbose=1, scenecut=150)
    if lookahead:
        kw["lookahead"] = lookahead
    harness.run_one_point(nets[0], nets[1], yuv, W, H, 12, QP, QP, **kw)                       # warm-up
    if not collector:                 # no collection of the interpreter's lands in one variant's timed frames and not in another's
        gc.collect()
        gc.disable()
    log = harness.run_one_point(nets[0], nets[1], yuv, W, H, frames, QP, QP, **kw)
    print(json.dumps({"enc_ms": 1e3 * log["avg_frame_encoding_time"], "i": log["i_frame_num"], "cuts": log["scene_cuts"],
                      "bpp": log["ave_all_frame_bpp"]}))


if len(sys.argv) > 1 and sys.argv[1] == "point":
    point(sys.argv[2], sys.argv[3], int(sys.argv[4]), int(sys.argv[5]), int(sys.argv[6]))
    sys.exit(0)

sys.path.insert(0, HERE)
import numpy as np
import torch
from opendcvc_amd import _lib, weights
from opendcvc_amd.entropy import PinnedBuffer

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 3
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(HERE, "profiles", "r17_lookahead.txt")
parent = sys.argv[3] if len(sys.argv) > 3 else None
CALLS = 300
dev = torch.device("cuda", 0)
L = _lib.lib()
P = lambda t: ctypes.c_void_p(t.data_ptr())
stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
lines = [f"frame lookahead, {torch.cuda.get_device_name(0)}"]


# ---------------------------------------------------------------------------------- 1. the kernels
def kernel_times(bh, bw):
    sets = max(2, -(-512 * 2 ** 20 // (2 * bh * bw * 2)))
    planes = torch.randint(-32768, 32767, (sets, 2, bh, bw), dtype=torch.int16, device=dev)       # (any uint16 is a sample)
    one = torch.randint(-32768, 32767, (2, 1, 1), dtype=torch.int16, device=dev)
    ws = torch.empty(L.dcvc_lookahead_ws_bytes(bh, bw), dtype=torch.uint8, device=dev)
    pinned = PinnedBuffer(64)
    out = ctypes.c_void_p(pinned.ptr)
    st, wsp = stream(), P(ws)
    ptr = [(P(planes[i, 0]), P(planes[i, 1])) for i in range(sets)]           # (nothing but the call between the two events)
    small = (P(one[0]), P(one[1]))
    call = lambda pair, h, w: L.dcvc_lookahead_cost(pair[0], pair[1], h, w, wsp, out, st)
    variants = [("operands not in a cache", lambda k: call(ptr[k % sets], bh, bw)),
                ("one pair over and over", lambda k: call(ptr[0], bh, bw)),
                ("1 x 1 (launch floor)", lambda k: call(small, 1, 1))]
    for _, fn in variants:
        for k in range(32):
            _lib.check(fn(k), "warm-up")
    torch.cuda.synchronize(dev)
    ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(CALLS)] for _ in variants]
    for k in range(CALLS):
        for vi, (_, fn) in enumerate(variants):
            a, b = ev[vi][k]
            a.record()
            rc = fn(k)
            b.record()
            _lib.check(rc, "dcvc_lookahead_cost")
        if k % 16 == 15:
            torch.cuda.synchronize(dev)
    torch.cuda.synchronize(dev)
    tiles = -(-bh // 8) * -(-bw // 8)
    lines.append(f"dcvc_lookahead_cost {bh} x {bw} plane ({tiles} tiles, {2 * bh * bw * 2 / 1e3:.0f} KB of operands): HIP events around "
                 f"the call's three launches, {CALLS} calls per variant, {sets} plane pairs")
    for (name, _), e in zip(variants, ev):
        t = np.asarray([a.elapsed_time(b) * 1e3 for a, b in e])
        q1, med, q3 = np.percentile(t, [25, 50, 75])
        lines.append(f"  {name:26s} median {med:7.2f} us  quartiles {q1:7.2f} .. {q3:7.2f}  min {t.min():7.2f}")


for shape in ((135, 240), (270, 480)):
    kernel_times(*shape)
    torch.cuda.empty_cache()

from opendcvc_amd.lookahead import Lookahead
la = Lookahead(dev, 4, 150)
x = [torch.rand((1, 3, 1088, 1920), device=dev).half() for _ in range(2)]
for k in range(8):
    la.push(x[k & 1])
t = []
for _ in range(CALLS):
    t0 = time.perf_counter()
    la.words(7, 6)
    t.append((time.perf_counter() - t0) * 1e6)
q1, med, q3 = np.percentile(t, [25, 50, 75])
lines.append(f"Lookahead.words at 1080p on an idle device (enqueue, stream synchronise, eight words read; host clock): median {med:7.2f} us  "
             f"quartiles {q1:7.2f} .. {q3:7.2f}")
del la, x
torch.cuda.empty_cache()

# ---------------------------------------------------------------------------------- 2. and 3. the harness, in child processes
import tempfile
tri = lambda k: k % 14 if k % 14 < 8 else 14 - k % 14            # forth and back: the generator's shift never wraps
tmp = tempfile.mkdtemp()
yuv = os.path.join(tmp, "steady.yuv")
with open(yuv, "wb") as f:
    cache = {}
    for k in range(FRAMES):
        if tri(k) not in cache:
            cache[tri(k)] = b"".join(p.tobytes() for p in weights.synthetic_frame_yuv420(H, W, tri(k), 0))
        f.write(cache[tri(k)])


def child(tree, lookahead, collector):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "point", tree, yuv, str(FRAMES), str(lookahead), str(collector)],
                       capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise SystemExit(f"child failed ({r.returncode}):\n{r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


variants = [("this tree, scenecut 150", HERE, 0), ("this tree, scenecut 150 + lookahead 4", HERE, 4)]
if parent:
    variants.insert(0, ("parent tree, scenecut 150", os.path.abspath(parent), 0))
for collector in (1, 0):
    got = {name: [] for name, _, _ in variants}
    for r in range(rounds):
        for name, tree, n in variants[r % len(variants):] + variants[:r % len(variants)]:      # (no variant keeps one place in the round)
            got[name].append(child(tree, n, collector))
            print(collector, name, got[name][-1], file=sys.stderr, flush=True)
    lines.append(f"harness, {W} x {H} fp16, {FRAMES} frames of material without a cut (qp {QP}), avg_frame_encoding_time over the frames "
                 f"behind the first ten; one fresh process per run after a 12-frame warm-up run, {rounds} rounds alternated, the order "
                 f"rotated round by round; garbage collector {'as it is' if collector else 'off during the timed run'}")
    for name, _, _ in variants:
        t = [r["enc_ms"] for r in got[name]]
        lines.append(f"  {name:40s} ms per frame: {'  '.join('%7.3f' % v for v in t)}   median {np.median(t):7.3f}  "
                     f"I frames {got[name][0]['i']}  cuts {got[name][0]['cuts']}  bpp {got[name][0]['bpp']:.5f}")
text = "\n".join(lines) + "\n"
print(text, end="")
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write(text)
os.remove(yuv)
os.rmdir(tmp)
