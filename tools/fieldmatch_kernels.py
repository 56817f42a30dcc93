"""Developer tool: launches of the film mode's kernels for a kernel trace (rocprofv3 --kernel-trace --stats -- python
tools/fieldmatch_kernels.py H W weave|idle): fp16, operands rotated through more than 512 MB, 200 launches per kernel after
warm-up.  weave: dcvc_field_match with a previous frame and dcvc_field_weave behind a word that reads 1; idle: dcvc_field_match
without a previous frame and dcvc_field_weave behind a word that reads 0.  The kernels' times are the trace's; this script
prints nothing but the launch count."""
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from opendcvc_amd import _lib

H, W, mode = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
dev = torch.device("cuda", 0)
L = _lib.lib()
P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
Hp, Wp = H + (-H) % 16, W + (-W) % 16
n = 3 * Hp * Wp
sets = -(-512 * 2 ** 20 // (2 * n)) + 2
fr = [torch.rand(n, dtype=torch.float16, device=dev).view(1, 3, Hp, Wp) for _ in range(sets)]
word = torch.tensor([1 if mode == "weave" else 0], dtype=torch.int32, device=dev)
need = L.dcvc_field_match_ws_bytes()
ws = torch.zeros(need + 8, dtype=torch.uint8, device=dev)
verdict = ctypes.c_void_p(ws.data_ptr() + need)
count = 0
for k in range(16 + 200):
    cur, prev, out = fr[k % sets], fr[(k + 1) % sets], fr[(k + 2) % sets]
    calls = [L.dcvc_field_match(_lib.F16, P(cur), P(prev) if mode == "weave" else None, Hp, Wp, H, W, 0, P(ws), verdict, st),
             L.dcvc_field_weave(_lib.F16, P(prev), Hp, Wp, H, W, 0, 2, P(word), P(out), st)]
    for rc in calls:
        _lib.check(rc, "launch")
    count += len(calls)
    if k % 16 == 15:
        torch.cuda.synchronize(dev)
torch.cuda.synchronize(dev)
print(f"{H} x {W} {mode}: {count} launches, the first {16 * len(calls)} are warm-up")
