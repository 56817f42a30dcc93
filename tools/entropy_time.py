"""Developer tool: the entropy mode of DMCI / DMC at 1080p, fp16, the bench's 32-frame GOP on one MI355X - entropy="host"
(the reference's stream, host rANS coder: the default) against entropy="device" (chunked payloads coded by the kernels of
csrc/dcvc_rans_dev.hip) with chunks of 256 / 512 / 1024 symbols, alternated round by round in one process after warm-up.
Per mode: sequential encode and decode time of a P frame (host clock around work that ends in a synchronise, median over
the GOP's P frames and the rounds), frames/s of the two-stage EncodeDecodePipeline over two GOPs, and the GOP's bpp; the
decoded pictures of every mode are compared with host mode's.
    python tools/entropy_time.py [rounds=3] [out=profiles/r08_device_entropy.txt]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from opendcvc_amd import weights
from opendcvc_amd.models import DMC, DMCI
from opendcvc_amd.pipeline import (EncodeDecodePipeline, SequenceDecoder, SequenceEncoder, load_yuv420_frame,
                                   use_two_entropy_coders)

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 3
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                                "profiles", "r08_device_entropy.txt")
H, W, GOP, QP = 1080, 1920, 32, 32
dev = torch.device("cuda", 0)
torch.set_grad_enabled(False)
torch.set_num_threads(1)
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
frames = []
for fi in range(GOP):
    yuv = [torch.from_numpy(a).to(dev) for a in weights.synthetic_frame_yuv420(H, W, fi, 0)]
    frames.append(load_yuv420_frame(*yuv, torch.float16))
MODES = [("host", None), ("device", 8), ("device", 9), ("device", 10)]


def set_mode(mode):
    for m in (ie, pe, idec, pdec):
        m.entropy = mode[0]
        if mode[1] is not None:
            m.chunk_log2 = mode[1]


def sequential(mode):
    """one GOP, encoder loop then decoder loop, every frame synchronised: (P encode times, P decode times, bytes, pictures)"""
    set_mode(mode)
    enc = SequenceEncoder(ie, pe, QP, intra_period=GOP, reset_interval=GOP)
    dec = SequenceDecoder(idec, pdec, H, W, two)
    pkts, te, td, pics = [], [], [], []
    for x in frames:
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        pkts.append(enc.encode(x))
        torch.cuda.synchronize(dev)
        te.append(time.perf_counter() - t0)
    for pkt in pkts:
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        pics.append(dec.decode(pkt))
        torch.cuda.synchronize(dev)
        td.append(time.perf_counter() - t0)
    assert all(p.chunked == (mode[0] == "device") for p in pkts)
    return te[1:], td[1:], sum(len(p.bit_stream) for p in pkts), pics


def pipelined(mode, n=2 * GOP):
    """frames/s of n frames through encoder and decoder as bench.py runs them (two threads, deferred decoder output)"""
    set_mode(mode)
    enc = SequenceEncoder(ie, pe, QP, intra_period=GOP, reset_interval=GOP)
    dec = SequenceDecoder(idec, pdec, H, W, two, defer_output=True)
    pipe = EncodeDecodePipeline(enc, dec, dev)
    done = []
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    pipe.run((frames[k % GOP] for k in range(n)), None, lambda x: done.append(1))
    torch.cuda.synchronize(dev)
    dt = time.perf_counter() - t0
    assert len(done) == n
    return n / dt


ref_pics = None
for mode in MODES:                                   # warm-up: code objects, graph captures, staging buffers of every mode
    pics = sequential(mode)[3]
    pipelined(mode, GOP)
    if ref_pics is None:
        ref_pics = [p.clone() for p in pics]
    else:
        assert all(torch.equal(a, b) for a, b in zip(pics, ref_pics)), f"{mode}: decoded pictures differ from host mode's"
res = {m: dict(enc=[], dec=[], fps=[], bytes=0) for m in MODES}
for _ in range(rounds):
    for mode in MODES:
        te, td, nbytes, _ = sequential(mode)
        res[mode]["enc"] += te
        res[mode]["dec"] += td
        res[mode]["bytes"] = nbytes
        res[mode]["fps"].append(pipelined(mode))
lines = [f"1080p YUV 4:2:0, fp16, 32-frame GOP (1 I + 31 P, qp {QP}), {torch.cuda.get_device_name(0)}; entropy modes alternated "
         f"round by round ({rounds} rounds) in one process after warm-up; host clock around synchronised work; decoded pictures "
         "of every mode bit-identical to host mode's",
         f"{'mode':22s} {'enc ms / P frame':>26s} {'dec ms / P frame':>26s} {'pipeline frames/s':>24s} {'GOP bpp':>9s} {'vs host':>8s}"]
host_bytes = res[MODES[0]]["bytes"]
for mode in MODES:
    r = res[mode]
    e, d, f = np.asarray(r["enc"]) * 1e3, np.asarray(r["dec"]) * 1e3, np.asarray(r["fps"])
    name = "host (reference stream)" if mode[0] == "host" else f"device, S = {1 << mode[1]}"
    lines.append(f"{name:22s} {np.median(e):8.3f} ({e.min():6.3f} - {e.max():6.3f}) {np.median(d):8.3f} ({d.min():6.3f} - {d.max():6.3f}) "
                 f"{np.median(f):8.1f} ({f.min():6.1f} - {f.max():6.1f}) {r['bytes'] * 8 / (GOP * H * W):9.5f} "
                 f"{100.0 * (r['bytes'] / host_bytes - 1):+7.2f}%")
text = "\n".join(lines) + "\n"
print(text, end="")
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write(text)
