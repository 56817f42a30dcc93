"""Developer tool: what the decoder-state digest costs on one MI355X, fp16.
1. dcvc_state_digest (two launches) between two HIP events on buffers of the size of the 1080p P-frame feature, the 1080p
   picture and the 4K feature, operands rotated call by call through buffer sets of more than 512 MB each, against an 8-byte
   call (two launches with nothing to do: the floor), the variants alternated call by call after warm-up.
2. The loops at 1080p on a 32-frame GOP with digests off, on and off again (the second 'off' shows the spread), alternated
   round by round in one process: the harness's sequential encode loop (every frame synchronised; the encoder waits for the
   digest's event there), the deferred-stream encode loop, the harness's sequential decode loop, the deferred-output decode
   loop and the two-stage EncodeDecodePipeline.
    python tools/digest_time.py [rounds=5] [out=profiles/r11_state_digest.txt]"""
import ctypes
import dataclasses
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from opendcvc_amd import _lib, weights
from opendcvc_amd.entropy import PinnedBuffer
from opendcvc_amd.models import DMC, DMCI
from opendcvc_amd.pipeline import (EncodeDecodePipeline, SequenceDecoder, SequenceEncoder, load_yuv420_frame,
                                   use_two_entropy_coders)

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                                "profiles", "r11_state_digest.txt")
CALLS = 300
dev = torch.device("cuda", 0)
torch.set_grad_enabled(False)
torch.set_num_threads(1)
L = _lib.lib()
lines = [f"decoder-state digest, {torch.cuda.get_device_name(0)}, fp16"]


# ---------------------------------------------------------------------------------- 1. the kernels
def kernel_times():
    shapes = [("1080p feature 136 x 240 x 256", 136 * 240 * 256), ("1080p picture 3 x 1088 x 1920", 3 * 1088 * 1920),
              ("4K feature 270 x 480 x 256", 270 * 480 * 256)]
    ws = torch.empty(L.dcvc_state_digest_ws_bytes(8 * _lib.DIGEST_PASS_WORDS), dtype=torch.uint8, device=dev)
    pinned = PinnedBuffer(16)
    out = ctypes.c_void_p(pinned.ptr)
    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(t):
        return L.dcvc_state_digest(ctypes.c_void_p(t.data_ptr()), t.numel() * t.element_size(), ctypes.c_void_p(ws.data_ptr()),
                                   0, 0, out, stream())

    variants = []
    for label, n in shapes:
        sets = -(-512 * 2 ** 20 // (2 * n)) + 1
        bufs = [torch.empty(n, dtype=torch.float16, device=dev).normal_() for _ in range(sets)]
        variants.append((label, 2 * n, sets, lambda k, bufs=bufs: call(bufs[k % len(bufs)])))
    small = torch.zeros(4, dtype=torch.float16, device=dev)
    variants.append(("8 bytes (launch floor)", 8, 1, lambda k: call(small)))
    for _, _, sets, fn in variants:
        for k in range(min(sets, 16)):
            _lib.check(fn(k), "warm-up")
    torch.cuda.synchronize(dev)
    ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(CALLS)] for _ in variants]
    for k in range(CALLS):
        for vi, v in enumerate(variants):
            a, b = ev[vi][k]
            a.record()
            rc = v[3](k)
            b.record()
            _lib.check(rc, "dcvc_state_digest")
        if k % 16 == 15:
            torch.cuda.synchronize(dev)
    torch.cuda.synchronize(dev)
    lines.append(f"dcvc_state_digest: HIP events around the call's two launches, {CALLS} calls per variant, alternated call by "
                 "call; operands rotated through more than 512 MB per variant")
    for (label, nbytes, sets, _), e in zip(variants, ev):
        t = np.asarray([a.elapsed_time(b) * 1e3 for a, b in e])
        q1, med, q3 = np.percentile(t, [25, 50, 75])
        lines.append(f"  {label:32s} {nbytes / 1e6:7.2f} MB  {sets:3d} sets  median {med:7.2f} us  quartiles {q1:7.2f} .. {q3:7.2f}  "
                     f"min {t.min():7.2f}  {nbytes / (med * 1e-6) / 1e12:5.2f} TB/s")
    del variants
    torch.cuda.empty_cache()


kernel_times()

# ---------------------------------------------------------------------------------- 2. the loops
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
tri = lambda k: k % 14 if k % 14 < 8 else 14 - k % 14            # forth and back: the generator's shift never wraps
planes = [[torch.from_numpy(a).to(dev) for a in weights.synthetic_frame_yuv420(H, W, tri(k), 0)] for k in range(GOP)]
frames = [load_yuv420_frame(*p, torch.float16) for p in planes]
torch.cuda.synchronize(dev)
KW = dict(intra_period=GOP, reset_interval=GOP)


def enc_sequential(on):
    enc = SequenceEncoder(ie, pe, QP, digest=on, **KW)
    pkts, te = [], []
    for p in planes:
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        pkts.append(enc.encode(load_yuv420_frame(*p, torch.float16)))
        torch.cuda.synchronize(dev)
        te.append(time.perf_counter() - t0)
    return te[1:], pkts


def enc_deferred(on):
    enc = SequenceEncoder(ie, pe, QP, defer_stream=True, digest=on, **KW)
    pkts = enc.encode(frames[0])
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for x in frames[1:]:
        pkts += enc.encode(x)
    pkts += enc.flush()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) / (GOP - 1), pkts


PKTS_ON = enc_sequential(True)[1]
PKTS = {True: PKTS_ON, False: [dataclasses.replace(p, digest=None) for p in PKTS_ON]}


def dec_sequential(on):
    dec = SequenceDecoder(idec, pdec, H, W, two)
    td = []
    for p in PKTS[on]:
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        dec.decode(p)
        torch.cuda.synchronize(dev)
        dec.check_digests()
        td.append(time.perf_counter() - t0)
    assert dec.digests_checked == (GOP if on else 0)
    return td[1:], None


def dec_deferred(on):
    dec = SequenceDecoder(idec, pdec, H, W, two, defer_output=True)
    dec.decode(PKTS[on][0])
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for p in PKTS[on][1:]:
        dec.decode(p)
    dec.flush()
    torch.cuda.synchronize(dev)
    assert dec.digests_checked == (GOP if on else 0)
    return (time.perf_counter() - t0) / (GOP - 1), None


def pipelined(on):
    enc = SequenceEncoder(ie, pe, QP, defer_stream=True, digest=on, **KW)
    dec = SequenceDecoder(idec, pdec, H, W, two, defer_output=True)
    pkts = []
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    EncodeDecodePipeline(enc, dec, dev).run(frames, on_packet=pkts.append)
    torch.cuda.synchronize(dev)
    assert dec.digests_checked == (GOP if on else 0)
    return GOP / (time.perf_counter() - t0), pkts


LOOPS = [("enc sequential", enc_sequential, "ms per P frame (loader + encode(), every frame synchronised)", 1e3),
         ("enc deferred", enc_deferred, "ms per P frame (one synchronisation at the end)", 1e3),
         ("dec sequential", dec_sequential, "ms per P frame (decode(), synchronise, check_digests())", 1e3),
         ("dec deferred", dec_deferred, "ms per P frame (one synchronisation at the end)", 1e3),
         ("pipeline", pipelined, "frames/s (encode + decode)", 1.0)]
VARIANTS = [("off", False), ("on", True), ("off2", False)]
base = [p.bit_stream for p in PKTS_ON]
for _, fn, _, _ in LOOPS:                                # warm-up of every variant; the packets must not depend on it
    for on in (False, True):
        pk = fn(on)[1]
        assert pk is None or ([p.bit_stream for p in pk] == base and [p.digest for p in pk] == [p.digest for p in PKTS[on]])
res = {(name, tag): [] for name, _, _, _ in LOOPS for tag, _ in VARIANTS}
for _ in range(rounds):
    for name, fn, _, _ in LOOPS:
        for tag, on in VARIANTS:
            r = fn(on)[0]
            res[(name, tag)] += r if isinstance(r, list) else [r]
lines.append(f"loops, {W} x {H}, {GOP}-frame GOP (1 I + {GOP - 1} P, qp {QP}), {rounds} rounds alternated in one process after warm-up; "
             "off2 = off once more (the spread); the packets' payloads are identical")
for name, _, unit, scale in LOOPS:
    med = {}
    for tag, _ in VARIANTS:
        t = np.asarray(res[(name, tag)]) * scale
        q1, med[tag], q3 = np.percentile(t, [25, 50, 75])
        lines.append(f"  {name:14s} {tag:4s} median {med[tag]:8.3f}  quartiles {q1:8.3f} .. {q3:8.3f}  {unit}")
    lines.append(f"  {name:14s} on against off: {100 * (med['on'] / med['off'] - 1):+.2f} %   off2 against off: "
                 f"{100 * (med['off2'] / med['off'] - 1):+.2f} %")
text = "\n".join(lines) + "\n"
print(text, end="")
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write(text)
