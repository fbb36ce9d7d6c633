"""dl_pnn_inner_fwd / dl_pnn_inner_bwd alone at B = 65,536, F = 26, E = 16, D1 = 400 (the C2 fields
and first layer), beside two yardsticks measured in the same run: dl_hbm_copy of 1 GiB (bench.py's HBM
yardstick) applied to each kernel's algorithmic bytes, and dl_vfma_probe (the chip's f32 vector FMA
rate, which the f32-input MFMA shares) applied to its counted FLOPs.  Launches for a kernel trace
(rocprofv3 --kernel-trace --stats -- python scripts/pnn_bench.py) and event-timed means; the operands
may stay in the Infinity Cache across these back-to-back launches.

--step: instead, the whole training step of the C2 dnn_pipeline (26 fields, E = 16, hidden 400 x 3,
B = 65,536, lazy tables, hipGraph replay) event-timed with pnn = None and "inner": the in-step cost.

FLOPs a sample (multiply-add = 2): forward 2 D1 F E (T); backward three times that (T again, de,
dtheta).  Algorithmic bytes: forward one read of the F E field columns, a read and a write of h[0]
and the sign bits; backward the fields, d, a read and a write of dx0's field columns."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deep_learning_amd import _lib  # noqa: E402
from deep_learning_amd._lib import call, ptr  # noqa: E402

B, F, E, D1, N = 65536, 26, 16, 400, 30


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


def kernels():
    s = _lib.stream_handle()
    g = torch.Generator(device="cuda").manual_seed(1)
    copy_bytes = 1 << 30
    src, dst = torch.zeros(copy_bytes // 4, device="cuda"), torch.zeros(copy_bytes // 4, device="cuda")
    t_cp = timed(lambda: call("dl_hbm_copy", ptr(src), ptr(dst), copy_bytes, s))
    rate = 2 * copy_bytes / t_cp / 1e6     # TB/s moved (read + write)
    print("dl_hbm_copy   %8.1f us  %d B read + written: %.2f TB/s" % (t_cp, copy_bytes, rate))
    blocks, iters = 256 * 16, 4096
    out = torch.zeros(blocks * 256, device="cuda")
    t_f = timed(lambda: call("dl_vfma_probe", ptr(out), out.numel(), blocks, iters, s))
    tflops = blocks * 256 * 32.0 * iters / t_f / 1e6
    print("dl_vfma_probe %8.1f us  %.1f TFLOP/s f32 vector FMA" % (t_f, tflops))
    del src, dst
    ld = (13 + F * E + 1 + 15) // 16 * 16
    x0 = torch.randn(B, ld, device="cuda", generator=g) * 0.3
    theta = torch.randn(D1 * F, device="cuda", generator=g) * 0.2
    c0 = torch.randn(B, D1, device="cuda", generator=g)
    C = c0.clone()
    d = torch.randn(B, D1, device="cuda", generator=g) / B
    ldb = 32
    bits = torch.zeros(B, ldb, dtype=torch.int16, device="cuda")
    dx0 = torch.zeros(B, F * E, device="cuda")
    grid = _lib.lib().dl_pnn_grid(B)
    slab = torch.zeros(grid, D1 * F, device="cuda")
    fwd = lambda: call("dl_pnn_inner_fwd", B, F, E, D1, ptr(x0), ld, 0, ptr(theta), ptr(C), D1, ptr(bits), ldb, s)
    bwd = lambda: call("dl_pnn_inner_bwd", B, F, E, D1, ptr(x0), ld, 0, ptr(theta), ptr(d), D1, ptr(dx0), F * E, 0,
                       ptr(slab), grid, s)
    ff = 2.0 * D1 * F * E * B
    bf = B * (F * E * 4 + 2 * D1 * 4 + (D1 + 15) // 16 * 2)
    bb = B * (3 * F * E * 4 + D1 * 4)
    for name, fn, nbytes, flops in (("dl_pnn_inner_fwd", fwd, bf, ff), ("dl_pnn_inner_bwd", bwd, bb, 3 * ff)):
        t = timed(fn)
        t_b, t_c = nbytes / rate / 1e6, flops / tflops / 1e6
        print("%-16s %8.1f us  %d B: %.1f us at the copy's rate; %.2f GFLOP: %.1f us at the FMA rate "
              "(%.1f TFLOP/s reached, %.0f%% of it; bound by %s)"
              % (name, t, nbytes, t_b, flops / 1e9, t_c, flops / t / 1e6, 100 * t_c / t,
                 "compute" if t_c > t_b else "bandwidth"))


def step():
    from deep_learning_amd.engine import CTREngine, ModelSpec
    from deep_learning_amd.synthetic import make_batch
    V = 1_000_000
    bs = [make_batch(B, cate_index_size=V, seed=i) for i in range(4)]
    for pnn in (None, "inner", None, "inner"):
        eng = CTREngine(ModelSpec("dnn_pipeline", C=13, S=26, E=16, cate_index_size=V, hidden=[400, 400, 400],
                                  pnn=pnn), max_batch=B, seed=1, adam="lazy")
        for i in range(6):
            eng.train_step(bs[i % 4], graph=True)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(20):
            eng.train_step(bs[i % 4], graph=True)
        e1.record()
        torch.cuda.synchronize()
        eng.check_error()
        print("dnn_pipeline C2 step, pnn=%-5s  %8.1f us a step (20 graph steps, host feed included)"
              % (pnn, e0.elapsed_time(e1) * 1e3 / 20))
        del eng


if __name__ == "__main__":
    step() if "--step" in sys.argv else kernels()
