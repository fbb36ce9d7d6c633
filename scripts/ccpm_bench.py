"""dl_ccpm_fwd / dl_ccpm_bwd alone at B = 65,536, F = 26, E = 16, filters (4, 4) (the C2 fields), beside two
yardsticks measured in the same run: dl_hbm_copy of 1 GiB (bench.py's HBM yardstick) applied to each
kernel's algorithmic bytes, and dl_vfma_probe (the chip's f32 vector FMA rate) applied to its counted
FLOPs.  Event-timed means; x0 and dx0 (27 MB each) may stay in the Infinity Cache across these
back-to-back launches.

--step: instead, the whole training step of the C2 dnn_pipeline (26 fields, E = 16, hidden 400 x 3,
B = 65,536, lazy tables, hipGraph replay) event-timed with ccpm_filters = () and (4, 4): the in-step cost.

Algorithmic bytes: forward one read of the F E field columns, 4 B a sample written; backward that read plus
a read and a write of dx0's field columns.  FLOPs a sample (multiply-add = 2): forward, per layer,
2 * 9 C_{l-1} C_l over the 4 H_l W_l positions the pool reads, plus 2 H_L W_L C_L; backward the forward's
again plus, per layer, at most 2 * 9 C_{l-1} C_l H_l W_l for dK and as much for da_{l-1} (one position a
window carries a gradient)."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deep_learning_amd import _lib  # noqa: E402
from deep_learning_amd._lib import call, ptr  # noqa: E402

B, F, E, FILTERS, N = 65536, 26, 16, (4, 4), 30


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


def counts():
    """(parameters, forward FLOPs, backward FLOPs) a sample."""
    h, w, c = E, F, 1
    n, ff, fb = 0, 0, 0
    for co in FILTERS:
        h, w = h // 2, w // 2
        n += (9 * c + 1) * co
        ff += 2 * 9 * c * co * 4 * h * w
        fb += 2 * 2 * 9 * c * co * h * w
        c = co
    return n + h * w * c, ff + 2 * h * w * c, 2 * ff + fb + 4 * h * w * c


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
    n, ff, fb = counts()
    fl = (_lib.C.c_int32 * 3)(*FILTERS)
    ld = (13 + F * E + 1 + 15) // 16 * 16
    x0 = torch.randn(B, ld, device="cuda", generator=g) * 0.1
    prm = torch.randn(n, device="cuda", generator=g) * 0.3
    dz = torch.randn(B, device="cuda", generator=g) / B
    z = torch.zeros(B, device="cuda")
    dx0 = torch.zeros(B, F * E, device="cuda")
    grid = _lib.lib().dl_ccpm_grid(B)
    slab = torch.zeros(grid, n, device="cuda")
    fwd = lambda: call("dl_ccpm_fwd", B, F, E, len(FILTERS), fl, ptr(x0), ld, 0, ptr(prm), None, ptr(z), s)
    bwd = lambda: call("dl_ccpm_bwd", B, F, E, len(FILTERS), fl, ptr(x0), ld, 0, ptr(prm), ptr(dz), ptr(dx0), F * E, 0,
                       ptr(slab), grid, s)
    bf, bb = B * F * E * 4 + B * 4, 3 * B * F * E * 4 + B * 4
    for name, fn, nbytes, flops in (("dl_ccpm_fwd", fwd, bf, B * ff), ("dl_ccpm_bwd", bwd, bb, B * fb)):
        t = timed(fn)
        t_b, t_c = nbytes / rate / 1e6, flops / tflops / 1e6
        print("F=%d E=%d %r %-11s %8.1f us  %d B: %.1f us at the copy's rate; %.2f GFLOP: %.1f us at the FMA rate "
              "(%.1f TFLOP/s reached, %.0f%% of it; bound by %s)"
              % (F, E, FILTERS, name, t, nbytes, t_b, flops / 1e9, t_c, flops / t / 1e6, 100 * t_c / t,
                 "compute" if t_c > t_b else "bandwidth"))


def step():
    from deep_learning_amd.engine import CTREngine, ModelSpec
    from deep_learning_amd.synthetic import make_batch
    V = 1_000_000
    bs = [make_batch(B, cate_index_size=V, seed=i) for i in range(4)]
    for fl in ((), FILTERS, (), FILTERS):
        eng = CTREngine(ModelSpec("dnn_pipeline", C=13, S=26, E=16, cate_index_size=V, hidden=[400, 400, 400],
                                  ccpm_filters=fl), max_batch=B, seed=1, adam="lazy")
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
        print("dnn_pipeline C2 step, ccpm_filters=%-6r  %8.1f us a step (20 graph steps, host feed included)"
              % (fl, e0.elapsed_time(e1) * 1e3 / 20))
        del eng


if __name__ == "__main__":
    step() if "--step" in sys.argv else kernels()
