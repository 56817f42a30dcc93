"""Developer tool: launches of the two deinterlacing filters for a kernel trace (rocprofv3 --kernel-trace --stats -- python
tools/deint_field_kernels.py H W): fp16, 200 launches per kernel after warm-up, alternated - dcvc_deinterlace with a previous
frame and dcvc_deinterlace_field with both neighbours - every launch on four buffers of its own out of a ring of more than
512 MB, so that neither runs out of what the other left in the cache.  The kernels' times are the trace's; this script prints
nothing but the launch count."""
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from opendcvc_amd import _lib

H, W = int(sys.argv[1]), int(sys.argv[2])
dev = torch.device("cuda", 0)
L = _lib.lib()
st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
Hp, Wp = H + (-H) % 16, W + (-W) % 16
n = 3 * Hp * Wp
sets = -(-512 * 2 ** 20 // (2 * n)) + 3
fr = [torch.rand(n, dtype=torch.float16, device=dev).view(1, 3, Hp, Wp) for _ in range(sets)]
f = lambda k: ctypes.c_void_p(fr[k % sets].data_ptr())
count = 0
for k in range(16 + 200):
    a, b = 8 * k, 8 * k + 4
    calls = [L.dcvc_deinterlace(_lib.F16, f(a), f(a + 1), Hp, Wp, H, W, 0, 2, None, f(a + 3), st),
             L.dcvc_deinterlace_field(_lib.F16, f(b + 1), f(b), f(b + 2), Hp, Wp, H, W, 0, 2, f(b + 3), st)]
    for rc in calls:
        _lib.check(rc, "launch")
    count += len(calls)
    if k % 16 == 15:
        torch.cuda.synchronize(dev)
torch.cuda.synchronize(dev)
print(f"{H} x {W}: {count} launches, the first {16 * len(calls)} are warm-up")
