"""Developer tool: what rate control's size estimate costs on one MI355X, fp16, and how close it is.
1. dcvc_rate_estimate (two launches) between two HIP events on the symbols of a 1080p and of a 4K P frame (2 parts; 30 % of
   the entries skipped), operands alternated call by call over buffer sets of more than 512 MB in all, against the same
   call on ONE frame's symbols (the encode path: the front run has just written them) and against a 128-symbol call (two
   launches with nothing to do: the floor), the variants alternated call by call after warm-up.
2. The harness's sequential encode loop at 1080p (every frame synchronised, host clock: loader + encode() of a P frame) with
   a RateController whose qp range is one value against the same loop without one, alternated round by round in one process:
   the packets are identical, the difference is the estimate and its feedback.
3. The deferred-stream encode loop (SequenceEncoder(defer_stream=True), one synchronisation at the end) and the two-stage
   EncodeDecodePipeline, off and on in the same way.
4. The estimate against the exact bytes of every frame of the GOP.
    python tools/rate_time.py [rounds=5] [out=profiles/r10_rate_control.txt]"""
import ctypes
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from opendcvc_amd import _lib, entropy, weights
from opendcvc_amd.entropy import PinnedBuffer
from opendcvc_amd.models import DMC, DMCI
from opendcvc_amd.pipeline import (EncodeDecodePipeline, SequenceDecoder, SequenceEncoder, load_yuv420_frame,
                                   use_two_entropy_coders)
from opendcvc_amd.ratecontrol import RateController

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                                "profiles", "r10_rate_control.txt")
CALLS = 300
dev = torch.device("cuda", 0)
torch.set_grad_enabled(False)
torch.set_num_threads(1)
L = _lib.lib()
P = lambda t: ctypes.c_void_p(t.data_ptr())
stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
lines = [f"rate control, {torch.cuda.get_device_name(0)}, fp16"]
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


ie, pe, idec, pdec = make(DMCI, "dmci"), make(DMC, "dmc"), make(DMCI, "dmci"), make(DMC, "dmc")


# ---------------------------------------------------------------------------------- 1. the kernels
def kernel_times(yh, yw, label):
    g, z = (entropy.cost_table(*pe.entropy_coder.tables[k]) for k in (pe._g_group, pe._z_group))
    gd, zd = (torch.from_numpy(t.view(np.int32)).to(dev) for t in (g, z))
    nsym, zhw = 64 * yh * yw, ((yh + 3) // 4) * ((yw + 3) // 4)
    nz = pe.z_channel * zhw
    sets = max(2, -(-512 * 2 ** 20 // (4 * nsym + nz)))
    rng = np.random.default_rng(1)

    def symbols(n):
        idx = np.where(rng.random((2, n)) < 0.3, 0xFF, rng.integers(0, 128, (2, n)))
        sym = np.clip(np.rint(rng.normal(0, 2, (2, n))), -128, 127).astype(np.int64)
        return torch.from_numpy(((sym << 8) | idx).astype(np.uint16).view(np.int16)).to(dev)

    packed = [symbols(nsym) for _ in range(min(sets, 4))]
    packed += [packed[k % 4].clone() for k in range(4, sets)]
    z8 = [torch.from_numpy(np.clip(np.rint(rng.normal(0, 3, nz)), -128, 127).astype(np.int8)).to(dev) for _ in range(2)]
    small = symbols(128)
    ws = torch.empty(L.dcvc_rate_estimate_ws_bytes(nsym, 2, nz), dtype=torch.uint8, device=dev)
    pinned = PinnedBuffer(64)
    out = ctypes.c_void_p(pinned.ptr)

    def call(p, n, zz, hw):
        return L.dcvc_rate_estimate(P(p), n, 2, P(gd), gd.shape[0], gd.shape[1], P(zz), zz.numel(), hw, P(zd), zd.shape[0],
                                    zd.shape[1], QP * pe.z_channel, P(ws), out, stream())

    variants = [("operands not in a cache", lambda k: call(packed[k % sets], nsym, z8[k & 1], zhw)),
                ("one frame over and over", lambda k: call(packed[0], nsym, z8[0], zhw)),
                ("128 symbols (launch floor)", lambda k: call(small, 128, z8[0][:128], 1))]
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
            _lib.check(rc, "dcvc_rate_estimate")
        if k % 16 == 15:
            torch.cuda.synchronize(dev)
    torch.cuda.synchronize(dev)
    lines.append(f"dcvc_rate_estimate {label}: 2 x {nsym} y symbols + {nz} z, HIP events around the call's two launches, {CALLS} calls "
                 f"per variant, {sets} buffer sets")
    for (name, _), e in zip(variants, ev):
        t = np.asarray([a.elapsed_time(b) * 1e3 for a, b in e])
        q1, med, q3 = np.percentile(t, [25, 50, 75])
        nbytes = 0 if name.startswith("128") else 4 * nsym + nz
        lines.append(f"  {name:28s} median {med:7.2f} us  quartiles {q1:7.2f} .. {q3:7.2f}  min {t.min():7.2f}  symbols {nbytes / 1e6:6.2f} MB  "
                     f"{nbytes / (med * 1e-6) / 1e12:5.2f} TB/s")


kernel_times(68, 120, "1080p")
kernel_times(135, 240, "4K")
torch.cuda.empty_cache()

# ---------------------------------------------------------------------------------- 2. - 4. the encode loops
tri = lambda k: k % 14 if k % 14 < 8 else 14 - k % 14            # forth and back: the generator's shift never wraps
planes = [[torch.from_numpy(a).to(dev) for a in weights.synthetic_frame_yuv420(H, W, tri(k), 0)] for k in range(GOP)]
frames = [load_yuv420_frame(*p, torch.float16) for p in planes]
torch.cuda.synchronize(dev)
KW = dict(intra_period=GOP, reset_interval=GOP)


def controller(on):
    """on: a controller that may not move (the packets stay those of the fixed qp); off: none, and no estimate"""
    ie.rate_estimate = pe.rate_estimate = False
    return dict(rate=RateController(0.05 * H * W, QP, qp_min=QP, qp_max=QP)) if on else {}


def sequential(on):
    enc = SequenceEncoder(ie, pe, QP, **controller(on), **KW)
    pkts, te = [], []
    for p in planes:
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        pkts.append(enc.encode(load_yuv420_frame(*p, torch.float16)))
        torch.cuda.synchronize(dev)
        te.append(time.perf_counter() - t0)
    return te[1:], pkts, enc


def deferred(on):
    enc = SequenceEncoder(ie, pe, QP, defer_stream=True, **controller(on), **KW)
    pkts = enc.encode(frames[0])
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for x in frames[1:]:
        pkts += enc.encode(x)
    pkts += enc.flush()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) / (GOP - 1), pkts, enc


def pipelined(on):
    enc = SequenceEncoder(ie, pe, QP, defer_stream=True, **controller(on), **KW)
    dec = SequenceDecoder(idec, pdec, H, W, two, defer_output=True)
    pkts = []
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    EncodeDecodePipeline(enc, dec, dev).run(frames, on_packet=pkts.append)
    torch.cuda.synchronize(dev)
    return GOP / (time.perf_counter() - t0), pkts, enc


LOOPS = [("sequential", sequential), ("deferred", deferred), ("pipeline", pipelined)]
base = [p.bit_stream for p in sequential(False)[1]]
for _, fn in LOOPS:                                      # warm-up of every variant; the packets must not depend on it
    for on in (False, True):
        assert [p.bit_stream for p in fn(on)[1]] == base
res = {(name, on): [] for name, _ in LOOPS for on in (False, True)}
for _ in range(rounds):
    for name, fn in LOOPS:
        for on in (False, True):
            r = fn(on)[0]
            res[(name, on)] += r if isinstance(r, list) else [r]
lines.append(f"encode loops, {W} x {H}, {GOP}-frame GOP (1 I + {GOP - 1} P, qp {QP}), {rounds} rounds alternated in one process after "
             f"warm-up; 'on' = a RateController held at qp {QP}: packets identical to 'off'")
for name, unit, scale in (("sequential", "ms per P frame (loader + encode(), every frame synchronised)", 1e3),
                          ("deferred", "ms per P frame (one synchronisation at the end)", 1e3),
                          ("pipeline", "frames/s (encode + decode)", 1.0)):
    off, on = (np.asarray(res[(name, o)]) * scale for o in (False, True))
    for tag, t in (("off", off), ("on", on)):
        q1, med, q3 = np.percentile(t, [25, 50, 75])
        lines.append(f"  {name:10s} {tag:3s} median {med:8.3f}  quartiles {q1:8.3f} .. {q3:8.3f}  {unit}")
    lines.append(f"  {name:10s} on against off: {100 * (np.median(on) / np.median(off) - 1):+.2f} %")
enc = sequential(True)[2]
est, got = np.asarray(enc.rc_est_bytes), np.asarray(enc.rc_bytes)
lines.append(f"estimate against the exact bytes (payload + container) of the {GOP} frames: total {est.sum()} against {got.sum()} bytes "
             f"({100 * (est.sum() / got.sum() - 1):+.4f} %), per frame {(est - got).min():+d} .. {(est - got).max():+d} bytes of "
             f"{got.min()} .. {got.max()}")
text = "\n".join(lines) + "\n"
print(text, end="")
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write(text)
