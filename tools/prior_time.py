"""Developer tool: time of the latent-side entries (csrc/dcvc_prior.hip) alone, fp16, force_zero_thres 0.12, at the DMC step
(2 groups, 68 x 120, C = 128), the DMCI step (4 groups, 68 x 120, C = 256) and the 4K DMC step (2 groups, 136 x 240, C = 128),
and of dcvc_compact_symbols at 2 x 522240 symbols, in one process: warm-up, then the entries of a shape alternated launch by
launch, each call between two HIP events; medians and quartiles over the calls.  Every call works on the next of several
buffer sets (more than 512 MB in all) so that no operand is still in a cache.  Scales are drawn as in
test_decoder_hand_off_compacted_on_the_device (exp(N(-2.4, 1)): ~4 in 10 positions kept at 0.12).  Only ABI entries are
called, so the file runs unchanged in a checkout of an older commit.
    python tools/prior_time.py [calls=200] [out=profiles/prior_time.txt]"""
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from opendcvc_amd import _lib, entropy

n_calls = int(sys.argv[1]) if len(sys.argv) > 1 else 200
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                                "profiles", "prior_time.txt")
dev = torch.device("cuda", 0)
L = _lib.lib()
P = lambda t: ctypes.c_void_p(t.data_ptr())
HP = lambda b: ctypes.c_void_p(b.ptr)
stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
THRES = 0.12
rng = np.random.default_rng(16)


class Set:
    """the operands of one step, laid out as the codecs pass them: scales / means are channel slices of one params buffer"""

    def __init__(self, groups, H, W, C, q_mode):
        f16 = lambda a: torch.from_numpy(a.astype(np.float32)).half().to(dev)
        self.params = f16(np.concatenate([rng.uniform(0.3, 3.0, (H, W, C)), np.exp(rng.normal(-2.4, 1.0, (H, W, C))),
                                          rng.normal(0, 2, (H, W, C))], axis=2))
        self.qsrc = self.params[:, :, :C] if q_mode == 0 else self.params
        self.scales, self.means = self.params[:, :, C:2 * C], self.params[:, :, 2 * C:]
        self.y, self.yhat, self.out = f16(rng.normal(0, 8, (H, W, C))), f16(rng.normal(0, 2, (H, W, C))), f16(np.zeros((H, W, C)))
        n = (C // groups) * H * W
        cap = (n + 15) // 16 * 16
        self.packed = torch.empty(n, dtype=torch.int16, device=dev)
        self.idx = torch.empty(n, dtype=torch.uint8, device=dev)
        self.sym = torch.randint(-128, 128, (cap,), dtype=torch.int8, device=dev)
        self.ws = torch.zeros(int(L.dcvc_prior_dec_compact_ws_bytes(H, W, C, groups)), dtype=torch.uint8, device=dev)
        self.cidx, self.cnt = torch.empty(cap, dtype=torch.uint8, device=dev), torch.zeros(4, dtype=torch.int32, device=dev)
        self.hidx, self.hcnt, self.hsym = entropy.PinnedBuffer(cap), entropy.PinnedBuffer(16), entropy.PinnedBuffer(cap)
        self.hsym.u8[:] = 3
        self.bytes = 2 * (self.params.numel() + 3 * H * W * C) + 2 * n + 3 * cap + self.ws.numel()


def step_group(groups, H, W, C, q_mode):
    """-> [(name, call(k))] in an order in which every call finds what it reads (the restores follow their index build), sets"""
    one = Set(groups, H, W, C, q_mode)
    sets = [one] + [Set(groups, H, W, C, q_mode) for _ in range(max(1, -(-512 * 2 ** 20 // one.bytes)) - 1)]
    ld = lambda t: t.stride(1)
    head = (_lib.F16, groups, 1)                       # step 1: y_hat of step 0 is read and carried over
    size = (H, W, C)
    yh = lambda s: (P(s.yhat), ld(s.yhat), P(s.out), ld(s.out))
    return [
        ("dcvc_prior_enc_step", lambda s: L.dcvc_prior_enc_step(
            *head, q_mode, P(s.y), ld(s.y), P(s.qsrc), ld(s.qsrc), P(s.scales), ld(s.scales), P(s.means), ld(s.means), *size, THRES,
            *yh(s), P(s.packed), stream())),
        ("dcvc_prior_dec_index", lambda s: L.dcvc_prior_dec_index(*head, P(s.scales), ld(s.scales), *size, THRES, P(s.idx), stream())),
        ("dcvc_prior_dec_restore", lambda s: L.dcvc_prior_dec_restore(*head, P(s.sym), P(s.means), ld(s.means), *size, *yh(s), stream())),
        ("dcvc_prior_dec_index_compact (2 launches)", lambda s: L.dcvc_prior_dec_index_compact(
            *head, P(s.scales), ld(s.scales), *size, THRES, P(s.idx), P(s.ws), HP(s.hidx), HP(s.hcnt), stream())),
        ("dcvc_prior_dec_restore_compact (2 launches)", lambda s: L.dcvc_prior_dec_restore_compact(
            *head, HP(s.hsym), P(s.idx), P(s.ws), P(s.means), ld(s.means), *size, *yh(s), stream())),
        ("dcvc_prior_dec_index_compact_dev (2 launches)", lambda s: L.dcvc_prior_dec_index_compact_dev(
            *head, P(s.scales), ld(s.scales), *size, THRES, P(s.idx), P(s.ws), P(s.cidx), P(s.cnt), stream())),
        ("dcvc_prior_dec_restore_compact_dev", lambda s: L.dcvc_prior_dec_restore_compact_dev(
            *head, P(s.sym), P(s.idx), P(s.ws), P(s.means), ld(s.means), *size, *yh(s), stream())),
        ("dcvc_prior_finish", lambda s: L.dcvc_prior_finish(_lib.F16, q_mode, P(s.out), ld(s.out), P(s.qsrc), ld(s.qsrc), *size, stream())),
    ], sets


class SymbolSet:
    def __init__(self, parts, n):
        a = rng.integers(-32768, 32767, (parts, n), dtype=np.int16)
        a = np.where(rng.random((parts, n)) < 0.6, (a & ~0xFF) | 0xFF, np.where((a & 0xFF) == 0xFF, a & ~1, a)).astype(np.int16)
        self.packed = torch.from_numpy(a).to(dev)
        self.out, self.cnt = entropy.PinnedBuffer(parts * n * 2), entropy.PinnedBuffer(4 * parts)
        self.dout, self.dcnt = torch.empty(parts * n, dtype=torch.int16, device=dev), torch.zeros(parts, dtype=torch.int32, device=dev)
        self.ws = torch.zeros(256 * parts, dtype=torch.int32, device=dev)
        self.bytes = 6 * parts * n


def symbol_group(parts, n):
    sets = [SymbolSet(parts, n) for _ in range(-(-512 * 2 ** 20 // (6 * parts * n)))]
    return [("dcvc_compact_symbols (2 launches)", lambda s: L.dcvc_compact_symbols(P(s.packed), n, parts, HP(s.out), HP(s.cnt), P(s.ws), stream())),
            ("dcvc_compact_symbols_dev (2 launches)", lambda s: L.dcvc_compact_symbols_dev(P(s.packed), n, parts, P(s.dout), P(s.dcnt), P(s.ws),
                                                                                           stream()))], sets


def measure(group, sets):
    for _, call in group:                                          # warm-up: code objects, every buffer set touched once
        for s in sets:
            _lib.check(call(s), "warm-up")
    torch.cuda.synchronize(dev)
    events = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n_calls)] for _ in group]
    for it in range(n_calls):
        for vi, (_, call) in enumerate(group):
            a, b = events[vi][it]
            a.record()
            rc = call(sets[(it * len(group) + vi) % len(sets)])
            b.record()
            _lib.check(rc, "call")
        if it % 16 == 15:
            torch.cuda.synchronize(dev)                            # (keeps the queue of events short)
    torch.cuda.synchronize(dev)
    return [np.asarray([a.elapsed_time(b) * 1e3 for a, b in ev]) for ev in events]      # microseconds


lines = []
for label, make in (("DMC step 2 x 68 x 120 x 128", lambda: step_group(2, 68, 120, 128, 0)),
                    ("DMCI step 4 x 68 x 120 x 256", lambda: step_group(4, 68, 120, 256, 1)),
                    ("4K DMC step 2 x 136 x 240 x 128", lambda: step_group(2, 136, 240, 128, 0)),
                    ("symbols 2 x 522240", lambda: symbol_group(2, 522240))):
    group, sets = make()
    lines.append(f"{label}, fp16, {len(sets)} buffer sets, {n_calls} calls per entry")
    for (name, _), t in zip(group, measure(group, sets)):
        q1, med, q3 = np.percentile(t, [25, 50, 75])
        lines.append(f"  {name:48s} median {med:8.2f} us  quartiles {q1:8.2f} .. {q3:8.2f}  min {t.min():8.2f}")
    del group, sets
    torch.cuda.empty_cache()
text = "\n".join([f"latent-side entries, {torch.cuda.get_device_name(0)}; HIP events around single calls, the entries of a shape alternated "
                  "call by call after warm-up, operands rotated over the buffer sets"] + lines) + "\n"
print(text, end="")
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write(text)
