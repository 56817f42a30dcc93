"""Developer tool: time of the resampler (csrc/dcvc_resize.hip, dcvc_resize_frame) per frame - 1080p -> 720p, 720p -> 1080p
and 2160p -> 1080p, fp16 and fp32, the three filters - in one process: warm-up, then the variants alternated batch by
batch, each batch of BATCH launches between two HIP events (a single launch of 10 us is shorter than the host needs to
enqueue it, so single launches would time the host); medians and quartiles of the per-launch time over the batches, and
bytes (the source's valid region read once + the padded output written once) over the median against the 6.3 TB/s a
streaming kernel can reach on an MI355X.  Every launch works on the next of several buffer sets (more than 512 MB in
all) so that no operand is still in a cache.  The entry is called directly on tensors and tables made beforehand.
RESIZE_TIME_ONLY=<text> keeps the variants whose name contains the text (for a run under a kernel trace).
    python tools/resize_time.py [batches=100] [out=profiles/r12_resize.txt]"""
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from opendcvc_amd import _lib
from opendcvc_amd.resize import FILTERS, Resampler, padded

n = int(sys.argv[1]) if len(sys.argv) > 1 else 100
BATCH = 8
ONLY = os.environ.get("RESIZE_TIME_ONLY", "")
L = _lib.lib()
P = lambda t: ctypes.c_void_p(t.data_ptr())
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                                "profiles", "r12_resize.txt")
ACHIEVABLE = 6.3e12
dev = torch.device("cuda", 0)
scaler = Resampler(dev)
SIZES = [((1080, 1920), (720, 1280)), ((720, 1280), (1080, 1920)), ((2160, 3840), (1080, 1920))]


def variants(size_in, size_out, dtype):
    """-> [(name, bytes, launch(k))], number of buffer sets"""
    (H, W), (HO, WO) = size_in, size_out
    Hp, Wp = padded(H, 16), padded(W, 16)
    es = torch.empty((), dtype=dtype).element_size()
    nbytes = 3 * (H * W + padded(HO, 16) * padded(WO, 16)) * es
    sets = max(2, -(-512 * 2 ** 20 // nbytes))
    frames = [torch.rand((1, 3, Hp, Wp), device=dev).to(dtype) for _ in range(sets)]
    outs = [torch.empty((1, 3, padded(HO, 16), padded(WO, 16)), dtype=dtype, device=dev) for _ in range(sets)]
    code = _lib.F16 if dtype == torch.float16 else _lib.F32
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    group = []
    for name in FILTERS:
        (fh, ch, kh), (fv, cv, kv) = scaler.tables(W, WO, name), scaler.tables(H, HO, name)
        tail = (P(fh), P(ch), kh, P(fv), P(cv), kv, st)
        calls = [(code, P(frames[k]), Hp, Wp, H, W, P(outs[k]), padded(HO, 16), padded(WO, 16), HO, WO) + tail for k in range(sets)]
        group.append((f"{W}x{H} -> {WO}x{HO} {name}", nbytes, lambda k, calls=calls: L.dcvc_resize_frame(*calls[k])))
    return group, sets


def measure(group, sets):
    for _, _, launch in group:                                     # warm-up: code objects, tables, every buffer set touched once
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
            torch.cuda.synchronize(dev)                            # (keeps the queue of events short)
    torch.cuda.synchronize(dev)
    return [np.asarray([a.elapsed_time(b) * 1e3 / BATCH for a, b in ev]) for ev in events]      # microseconds per launch


lines = []
for dtype, tag in ((torch.float16, "fp16"), (torch.float32, "fp32")):
    for size_in, size_out in SIZES:
        group, sets = variants(size_in, size_out, dtype)
        group = [g for g in group if ONLY in f"{tag} {g[0]}"]
        if not group:
            continue
        lines.append(f"{tag}, {sets} buffer sets, {n} batches of {BATCH} launches per variant")
        for (name, nbytes, _), t in zip(group, measure(group, sets)):
            q1, med, q3 = np.percentile(t, [25, 50, 75])
            rate = nbytes / (med * 1e-6)
            lines.append(f"  {name:36s} median {med:8.2f} us  quartiles {q1:8.2f} .. {q3:8.2f}  min {t.min():8.2f}  "
                         f"{nbytes / 1e6:7.2f} MB  {rate / 1e9:7.1f} GB/s = {100 * rate / ACHIEVABLE:5.1f} % of 6.3 TB/s")
        del group
        torch.cuda.empty_cache()
text = "\n".join([f"dcvc_resize_frame, {torch.cuda.get_device_name(0)}; HIP events around batches of {BATCH} launches, variants alternated "
                  "batch by batch after warm-up, time per launch; bytes = the source's valid region read once + the padded output "
                  "written once"] + lines) + "\n"
print(text, end="")
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write(text)
