"""dl_cross_fwd / dl_cross_bwd alone at the C2 dnn tower-input shape (B = 65,536, D = 429 = 13 + 26 * 16,
L = 2) beside dl_hbm_copy of 1 GiB (bench.py's measured HBM yardstick): launches for a kernel trace
(rocprofv3 --kernel-trace --stats -- python scripts/cross_bench.py) and event-timed means.
Algorithmic bytes: forward one read of x0's D columns; backward that plus a read and a write of
dx0's columns."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deep_learning_amd import _lib  # noqa: E402
from deep_learning_amd._lib import call, ptr  # noqa: E402

B, D, L, N = 65536, 429, 2, 50
dense = 13
ld = (D + 1 + 15) // 16 * 16
dx_cols = D - dense
dx_ld = (dx_cols + 3) // 4 * 4
s = _lib.stream_handle()
g = torch.Generator(device="cuda").manual_seed(1)
x0 = torch.randn(B, ld, device="cuda", generator=g) * 0.01
prm = torch.randn((2 * L + 1) * D, device="cuda", generator=g) * 0.05
dz = torch.randn(B, device="cuda", generator=g) / B
sv, zc = torch.zeros(B, L, device="cuda"), torch.zeros(B, device="cuda")
dx0 = torch.zeros(B, dx_ld, device="cuda")
grid = _lib.lib().dl_cross_grid(B)
slab = torch.zeros(grid, (2 * L + 1) * D, device="cuda")
copy_bytes = 1 << 30
src, dst = torch.zeros(copy_bytes // 4, device="cuda"), torch.zeros(copy_bytes // 4, device="cuda")


def timed(fn, n=N):
    for _ in range(5):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


fwd = lambda: call("dl_cross_fwd", B, D, L, ptr(x0), ld, ptr(prm), ptr(sv), ptr(zc), s)
bwd = lambda: call("dl_cross_bwd", B, D, L, ptr(x0), ld, ptr(prm), ptr(sv), ptr(dz), ptr(dx0), dx_ld, 0, dx_cols,
                   ptr(slab), grid, s)
cp = lambda: call("dl_hbm_copy", ptr(src), ptr(dst), copy_bytes, s)
fb, bb = B * D * 4, B * D * 4 + 2 * B * dx_cols * 4
t_cp = timed(cp)
rate = 2 * copy_bytes / t_cp / 1e6     # TB/s moved (read + write)
print("dl_hbm_copy  %7.1f us  %d B read + written: %.2f TB/s" % (t_cp, copy_bytes, rate))
for name, fn, nbytes in (("dl_cross_fwd", fwd, fb), ("dl_cross_bwd", bwd, bb)):
    t = timed(fn)
    print("%-12s %7.1f us  algorithmic %d B: %.1f us at the copy's rate" % (name, t, nbytes, nbytes / rate / 1e6))
