"""Developer tool: launches of the deinterlacer's kernels for a kernel trace (rocprofv3 --kernel-trace --stats -- python
tools/deint_kernels.py H W filter|pass): fp16, operands rotated through more than 512 MB, 200 launches per kernel after warm-up.
filter: dcvc_deinterlace with and without a previous frame (no decision word) and dcvc_comb_detect with one; pass:
dcvc_deinterlace behind a decision word that reads 0 and dcvc_comb_detect without a previous frame.  The kernels' times are
the trace's; this script prints nothing but the launch count."""
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
zero = torch.zeros(1, dtype=torch.int32, device=dev)
ws = torch.zeros(L.dcvc_comb_ws_bytes() + 8, dtype=torch.uint8, device=dev)
verdict = ctypes.c_void_p(ws.data_ptr() + L.dcvc_comb_ws_bytes())
count = 0
for k in range(16 + 200):
    cur, prev, out = fr[k % sets], fr[(k + 1) % sets], fr[(k + 2) % sets]
    if mode == "filter":
        calls = [L.dcvc_deinterlace(_lib.F16, P(cur), P(prev), Hp, Wp, H, W, 0, 2, None, P(out), st),
                 L.dcvc_deinterlace(_lib.F16, P(cur), None, Hp, Wp, H, W, 0, 2, None, P(out), st),
                 L.dcvc_comb_detect(_lib.F16, P(cur), P(prev), Hp, Wp, H, W, 0, P(ws), verdict, st)]
    else:
        calls = [L.dcvc_deinterlace(_lib.F16, P(cur), P(prev), Hp, Wp, H, W, 0, 2, P(zero), P(out), st),
                 L.dcvc_comb_detect(_lib.F16, P(cur), None, Hp, Wp, H, W, 0, P(ws), verdict, st)]
    for rc in calls:
        _lib.check(rc, "launch")
    count += len(calls)
    if k % 16 == 15:
        torch.cuda.synchronize(dev)
torch.cuda.synchronize(dev)
print(f"{H} x {W} {mode}: {count} launches, the first {16 * len(calls)} are warm-up")
