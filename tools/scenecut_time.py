"""Developer tool: what scene-cut detection costs on one MI355X, fp16.
1. dcvc_frame_analyze (three launches) between two HIP events at 1088 x 1920 and 2160 x 3840: operands alternated call by
   call over buffer sets of more than 512 MB in all (nothing still in a cache), against the same call on ONE frame (the
   encode path: the loader has just written the frame) and against an 8 x 8 call (three launches with nothing to do: the
   floor), the variants alternated call by call after warm-up; luma bytes over the median against 6.3 TB/s.
2. The harness's sequential encode loop at 1080p (every frame synchronised, host clock: loader + encode() of a P frame) with
   scenecut 150 against the same loop with it off, alternated round by round in one process, on material without a cut
   (the synthetic texture moving forth and back); the packets of both must be identical.
3. The deferred-stream encode loop (SequenceEncoder(defer_stream=True), frames prepared up front, one synchronisation at
   the end) with it off, with it on and the frames' `ready` event passed, and with it on without the event.
    python tools/scenecut_time.py [rounds=5] [out=profiles/r09_scenecut.txt]"""
import ctypes
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from opendcvc_amd import _lib, weights
from opendcvc_amd.entropy import PinnedBuffer
from opendcvc_amd.models import DMC, DMCI
from opendcvc_amd.pipeline import SequenceEncoder, load_yuv420_frame, use_two_entropy_coders

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                                "profiles", "r09_scenecut.txt")
ACHIEVABLE = 6.3e12
CALLS = 300
dev = torch.device("cuda", 0)
torch.set_grad_enabled(False)
torch.set_num_threads(1)
L = _lib.lib()
P = lambda t: ctypes.c_void_p(t.data_ptr())
stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
lines = [f"scene-cut detection, {torch.cuda.get_device_name(0)}, fp16"]


# ---------------------------------------------------------------------------------- 1. the kernels
def kernel_times(H, W):
    sets = max(2, -(-512 * 2 ** 20 // (H * W * 2)))
    luma = [torch.rand((H, W), device=dev).half() for _ in range(sets)]
    small = torch.rand((8, 8), device=dev).half()
    low = [torch.empty((H // 8, W // 8), dtype=torch.uint16, device=dev) for _ in range(2)]
    low_small = [torch.empty((1, 1), dtype=torch.uint16, device=dev) for _ in range(2)]
    ws = torch.empty(L.dcvc_frame_analysis_ws_bytes(H, W), dtype=torch.uint8, device=dev)
    pinned = PinnedBuffer(32)
    out = ctypes.c_void_p(pinned.ptr)

    def call(x, h, w, planes, k):
        return L.dcvc_frame_analyze(_lib.F16, P(x), w, h, w, P(planes[(k + 1) & 1]), P(planes[k & 1]), P(ws), out, stream())

    variants = [("operands not in a cache", lambda k: call(luma[k % sets], H, W, low, k)),
                ("one frame over and over", lambda k: call(luma[0], H, W, low, k)),
                ("8 x 8 (launch floor)", lambda k: call(small, 8, 8, low_small, k))]
    for _, fn in variants:
        for k in range(sets):
            _lib.check(fn(k), "warm-up")
    torch.cuda.synchronize(dev)
    ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(CALLS)] for _ in variants]
    for k in range(CALLS):
        for vi, (_, fn) in enumerate(variants):
            a, b = ev[vi][k]
            a.record()
            rc = fn(k)
            b.record()
            _lib.check(rc, "dcvc_frame_analyze")
        if k % 16 == 15:
            torch.cuda.synchronize(dev)
    torch.cuda.synchronize(dev)
    lines.append(f"dcvc_frame_analyze {W} x {H}: HIP events around the call's three launches, {CALLS} calls per variant, {sets} buffer sets")
    for (name, _), e in zip(variants, ev):
        t = np.asarray([a.elapsed_time(b) * 1e3 for a, b in e])
        q1, med, q3 = np.percentile(t, [25, 50, 75])
        nbytes = 0 if name.startswith("8 x 8") else H * W * 2
        rate = nbytes / (med * 1e-6)
        lines.append(f"  {name:26s} median {med:7.2f} us  quartiles {q1:7.2f} .. {q3:7.2f}  min {t.min():7.2f}  luma {nbytes / 1e6:6.2f} MB  "
                     f"{rate / 1e12:5.2f} TB/s = {100 * rate / ACHIEVABLE:5.1f} % of 6.3 TB/s")
    # one call from the host's side: enqueue + the one synchronisation, as FrameAnalyzer.analyze pays it
    from opendcvc_amd.analysis import FrameAnalyzer
    an = FrameAnalyzer(dev)
    x = luma[0].view(1, 1, H, W)
    for _ in range(20):
        an.analyze(x)
    torch.cuda.synchronize(dev)
    t = []
    for _ in range(CALLS):
        t0 = time.perf_counter()
        an.analyze(x)
        t.append((time.perf_counter() - t0) * 1e6)
    q1, med, q3 = np.percentile(t, [25, 50, 75])
    lines.append(f"  FrameAnalyzer.analyze on an idle device (event, enqueue, stream synchronise; host clock): median {med:7.2f} us  "
                 f"quartiles {q1:7.2f} .. {q3:7.2f}")


for hw in ((1088, 1920), (2160, 3840)):
    kernel_times(*hw)
    torch.cuda.empty_cache()

# ---------------------------------------------------------------------------------- 2. and 3. the encode loops
H, W, GOP, QP = 1080, 1920, 32, 32
two = use_two_entropy_coders(H, W)


def make(cls, name):
    m = cls()
    m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in weights.make_state_dict(name, 1234).items()})
    m.to(dev).eval()
    m.update(0.12)
    m.half()
    m.set_use_two_entropy_coders(two)
    return m


ie, pe = make(DMCI, "dmci"), make(DMC, "dmc")
tri = lambda k: k % 14 if k % 14 < 8 else 14 - k % 14            # forth and back: the generator's shift never wraps
planes = [[torch.from_numpy(a).to(dev) for a in weights.synthetic_frame_yuv420(H, W, tri(k), 0)] for k in range(GOP)]
frames = [load_yuv420_frame(*p, torch.float16) for p in planes]
ready = torch.cuda.Event()
ready.record(torch.cuda.current_stream())
torch.cuda.synchronize(dev)
KW = dict(intra_period=GOP, reset_interval=GOP)


def sequential(scenecut):
    """the harness's loop (run_one_point): -> (encode times of the P frames, packets)"""
    enc = SequenceEncoder(ie, pe, QP, scenecut=scenecut, **KW)
    pkts, te = [], []
    for p in planes:
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        pkts.append(enc.encode(load_yuv420_frame(*p, torch.float16)))
        torch.cuda.synchronize(dev)
        te.append(time.perf_counter() - t0)
    assert enc.scene_cuts == [] and [p.is_i for p in pkts] == [True] + [False] * (GOP - 1)
    return te[1:], pkts


def deferred(scenecut, event):
    """-> (seconds per frame over the GOP's P frames, packets)"""
    enc = SequenceEncoder(ie, pe, QP, defer_stream=True, scenecut=scenecut, **KW)
    pkts = enc.encode(frames[0], ready=event) if scenecut else enc.encode(frames[0])
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for x in frames[1:]:
        pkts += enc.encode(x, ready=event) if scenecut else enc.encode(x)
    pkts += enc.flush()
    torch.cuda.synchronize(dev)
    dt = time.perf_counter() - t0
    assert enc.scene_cuts == []
    return dt / (GOP - 1), pkts


SEQ = [("scenecut off", 0), ("scenecut 150", 150)]
DEF = [("scenecut off", 0, None), ("scenecut 150, ready event passed", 150, ready), ("scenecut 150, no event", 150, None)]
base = sequential(0)[1]                                # warm-up of every variant; the packets must not depend on it
for _, sc in SEQ:
    assert [p.bit_stream for p in sequential(sc)[1]] == [p.bit_stream for p in base]
for _, sc, evt in DEF:
    assert [p.bit_stream for p in deferred(sc, evt)[1]] == [p.bit_stream for p in base]
seq = {name: [] for name, _ in SEQ}
dfr = {name: [] for name, _, _ in DEF}
for _ in range(rounds):
    for name, sc in SEQ:
        seq[name] += sequential(sc)[0]
    for name, sc, evt in DEF:
        dfr[name].append(deferred(sc, evt)[0])
lines.append(f"sequential encode loop of the harness, {W} x {H}, {GOP}-frame GOP (1 I + {GOP - 1} P, qp {QP}), material without a cut, "
             f"{rounds} rounds alternated in one process after warm-up; packets identical with and without scenecut")
med = {}
for name, _ in SEQ:
    t = np.asarray(seq[name]) * 1e3
    q1, med[name], q3 = np.percentile(t, [25, 50, 75])
    lines.append(f"  {name:34s} loader + encode() per P frame: median {med[name]:7.3f} ms  quartiles {q1:7.3f} .. {q3:7.3f}  min {t.min():7.3f}")
d = med["scenecut 150"] - med["scenecut off"]
lines.append(f"  analysis and its synchronisation: {1e3 * d:+.1f} us per P frame = {100 * d / med['scenecut off']:+.2f} % of the encode time")
lines.append(f"deferred-stream encode loop (frames prepared up front, one synchronisation at the end), ms per P frame, {rounds} rounds")
for name, _, _ in DEF:
    t = np.asarray(dfr[name]) * 1e3
    lines.append(f"  {name:34s} median {np.median(t):7.3f} ms  range {t.min():7.3f} .. {t.max():7.3f}  "
                 f"({100 * (np.median(t) / np.median(np.asarray(dfr['scenecut off']) * 1e3) - 1):+.2f} %)")
text = "\n".join(lines) + "\n"
print(text, end="")
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write(text)
