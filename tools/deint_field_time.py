"""Developer tool: what field-rate deinterlacing (docs/deinterlace.md, "Field-rate output") costs on one MI355X, fp16.
1. dcvc_deinterlace_field with both neighbours against dcvc_deinterlace with a previous frame - both move three frames - between
   two HIP events at 1080p and 2160p, the entries alternated call by call after warm-up, EVERY call on four buffers of its
   own out of a ring of more than 512 MB (no call reads what the call before it touched: two entries alternated on the same
   operands would time the second one out of the cache); the existing filter is timed TWICE per round, so that the gap
   between its two series is the spread the other gap is held against.  Each against its traffic floor at 6.3 TB/s.
2. Deinterlacer(rate="field").fields(): wall time per call on an idle stream, the launches only (nothing is waited for).
3. The harness on an interlaced 1920 x 1080 clip: run_one_point's avg_frame_encoding_time / avg_frame_decoding_time (per
   PICTURE, behind the first ten) with --deinterlace on, on + --deint-rate field, and on again (the spread), alternated round
   by round in one process.
    python tools/deint_field_time.py [rounds=5] [out=profiles/r24_field_rate.txt] [harness-only | kernels-only]"""
import ctypes
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from opendcvc_amd import _lib, harness, weights
from opendcvc_amd.deinterlace import Deinterlacer

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                                "profiles", "r24_field_rate.txt")
only = sys.argv[3] if len(sys.argv) > 3 else ""
CALLS = 300
STREAM_TBS = 6.3               # what a streaming kernel reaches here (README)
dev = torch.device("cuda", 0)
torch.set_grad_enabled(False)
torch.set_num_threads(1)
L = _lib.lib()
lines = [f"field-rate deinterlacing, {torch.cuda.get_device_name(0)}, fp16"]
P = lambda t: ctypes.c_void_p(t.data_ptr())
stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
pad = lambda n: n + (-n) % 16


# ---------------------------------------------------------------------------------- 1. the kernels, 2. the object
def kernel_times(H, W):
    Hp, Wp = pad(H), pad(W)
    n = 3 * Hp * Wp
    sets = -(-512 * 2 ** 20 // (2 * n)) + 3
    fr = [torch.rand(n, dtype=torch.float16, device=dev).view(1, 3, Hp, Wp) for _ in range(sets)]
    f = lambda k: P(fr[k % sets])

    def frame_rate(c):                                       # call c of the run: sets 4 c .. 4 c + 3 are its own
        return L.dcvc_deinterlace(_lib.F16, f(4 * c), f(4 * c + 1), Hp, Wp, H, W, 0, 2, None, f(4 * c + 3), stream())

    def field_rate(c):
        return L.dcvc_deinterlace_field(_lib.F16, f(4 * c + 1), f(4 * c), f(4 * c + 2), Hp, Wp, H, W, 0, 2, f(4 * c + 3), stream())

    frame = 3 * H * W * 2
    variants = [("dcvc_deinterlace, prev", 3 * frame, frame_rate), ("dcvc_deinterlace_field, both", 3 * frame, field_rate),
                ("dcvc_deinterlace, prev (again)", 3 * frame, frame_rate)]
    for _, _, fn in variants:
        for k in range(min(sets, 16)):
            _lib.check(fn(k), "warm-up")
    torch.cuda.synchronize(dev)
    ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(CALLS)] for _ in variants]
    for k in range(CALLS):
        for vi, v in enumerate(variants):
            a, b = ev[vi][k]
            a.record()
            rc = v[2](len(variants) * k + vi)
            b.record()
            _lib.check(rc, v[0])
        if k % 16 == 15:
            torch.cuda.synchronize(dev)
    torch.cuda.synchronize(dev)
    lines.append(f"{W} x {H}: HIP events around each launch, {CALLS} calls per entry, alternated call by call; every call on four "
                 f"sets of its own out of {sets} ({sets * n * 2 / 2 ** 20:.0f} MB); 4:2:0 chroma lines")
    med = []
    for (label, nbytes, _), e in zip(variants, ev):
        t = np.asarray([a.elapsed_time(b) * 1e3 for a, b in e])
        q1, m, q3 = np.percentile(t, [25, 50, 75])
        med.append(m)
        floor = nbytes / (STREAM_TBS * 1e12) * 1e6
        lines.append(f"  {label:32s} {nbytes / 1e6:7.2f} MB  median {m:7.2f} us  quartiles {q1:7.2f} .. {q3:7.2f}  min {t.min():7.2f}"
                     f"  floor {floor:6.2f} us  x{m / floor:6.1f}  {nbytes / (m * 1e-6) / 1e12:5.2f} TB/s")
    lines.append(f"  field - frame: {med[1] - med[0]:+.2f} us   frame (again) - frame, the spread: {med[2] - med[0]:+.2f} us")

    di = Deinterlacer(dev, "on", "tff", 2, rate="field")
    for k in range(32):
        di.fields(fr[k % sets], (H, W))
    torch.cuda.synchronize(dev)
    t = []
    for k in range(CALLS):
        t0 = time.perf_counter()
        di.fields(fr[k % sets], (H, W))
        t.append((time.perf_counter() - t0) * 1e6)
        if k % 16 == 15:
            torch.cuda.synchronize(dev)
    q1, m, q3 = np.percentile(t, [25, 50, 75])
    lines.append(f"  Deinterlacer(rate='field').fields(): host time per call (two outputs' allocation and two launches; nothing is "
                 f"waited for)  median {m:7.2f} us  quartiles {q1:7.2f} .. {q3:7.2f}  min {min(t):7.2f}")
    del di, variants, fr
    torch.cuda.empty_cache()


def finish():
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)


if only != "harness-only":
    kernel_times(1080, 1920)
    kernel_times(2160, 3840)
if only == "kernels-only":
    finish()
    sys.exit(0)

# ---------------------------------------------------------------------------------- 3. the harness
H, W, FRAMES = 1080, 1920, 30
nets = harness.load_nets(None, None, 0.12, False, "cuda:0")
tri = lambda k: k % 14 if k % 14 < 8 else 14 - k % 14            # forth and back: the generator's shift never wraps
with tempfile.TemporaryDirectory() as d:
    content = [weights.synthetic_frame_yuv420(H, W, k, 0) for k in range(8)]
    src = os.path.join(d, "interlaced.yuv")
    with open(src, "wb") as f:
        for k in range(FRAMES):                                   # field k of the content: the even lines of frame k, the odd of k + 1
            first, second = content[tri(k)], content[tri(k + 1)]
            for a, b in zip(first, second):
                plane = np.array(a)
                plane[1::2] = b[1::2]
                f.write(plane.tobytes())

    def point(kw):
        log = harness.run_one_point(*nets, src, W, H, FRAMES, 32, 32, verbose=1, deinterlace="on", **kw)
        return (log["avg_frame_encoding_time"] * 1e3, log["avg_frame_decoding_time"] * 1e3, log["ave_all_frame_bpp"],
                log["i_frame_num"] + log["p_frame_num"])

    VARIANTS = [("on", {}), ("field", {"deint_rate": "field"}), ("on2", {})]
    for _, kw in VARIANTS[:2]:
        point(kw)                                                 # warm-up
    res = {tag: [] for tag, _ in VARIANTS}
    for _ in range(rounds):
        for tag, kw in VARIANTS:
            res[tag].append(point(kw))
    lines.append(f"harness, {W} x {H}, {FRAMES} interlaced frames (1 I + P, qp 32, fp16), --deinterlace on: avg_frame_encoding_time / "
                 f"avg_frame_decoding_time per PICTURE over the pictures behind the first ten, {rounds} rounds alternated in one "
                 f"process after warm-up; on2 = on once more (the spread); pictures on {res['on'][0][3]} field {res['field'][0][3]}; "
                 f"bpp per picture on {res['on'][0][2]:.4f} field {res['field'][0][2]:.4f} (random-weight nets: the bpp says nothing "
                 f"about a trained model)")
    for col, what in ((0, "encode"), (1, "decode")):
        med = {}
        for tag, _ in VARIANTS:
            t = np.asarray([r[col] for r in res[tag]])
            med[tag] = float(np.median(t))
            lines.append(f"  {what} {tag:5s} median {med[tag]:7.3f}  min {t.min():7.3f}  max {t.max():7.3f}  ms per picture")
        lines.append(f"  {what} field - on: {(med['field'] - med['on']) * 1e3:+.1f} us   on2 - on: {(med['on2'] - med['on']) * 1e3:+.1f} us per picture")
finish()
