"""dl_autoint_fwd / dl_autoint_bwd alone at B = 65,536, F = 26, E = 16 (the C2 fields), (L, Hn, D) = (2, 2, 16)
and (3, 4, 32), beside three yardsticks measured in the same run: dl_hbm_copy of 1 GiB (bench.py's HBM
yardstick) applied to each kernel's algorithmic bytes, dl_mfma_f32_probe (the chip's v_mfma_f32_16x16x4_f32
rate) and dl_vfma_probe (its f32 vector FMA rate) applied to the counted FLOPs.  Event-timed means.

--step: instead, the whole training step of the C2 dnn_pipeline (26 fields, E = 16, hidden 400 x 3,
B = 65,536, lazy tables, hipGraph replay) event-timed with autoint_layers = 0 and (2, 2, 16), two alternating
rounds: the in-step cost.

FLOPs a sample (multiply-add = 2): forward, a layer, 2 F D_{l-1} 4 D for the projections and 4 F^2 D for the
scores and A V; backward the forward again plus twice that.  Algorithmic bytes: forward one read of the F E
field columns and 4 B a sample written; backward that read plus a read and a write of dx0's field columns;
the weights stay in L1 / L2."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deep_learning_amd import _lib  # noqa: E402
from deep_learning_amd._lib import call, ptr  # noqa: E402

B, F, E, N = 65536, 26, 16, 10
SHAPES = ((2, 2, 16), (3, 4, 32))


def timed(fn, n=N, warm=2):
    for _ in range(warm):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


def fwd_flops(L, D):
    return sum(2.0 * F * (D if l else E) * 4 * D + 4.0 * F * F * D for l in range(L))


def kernels():
    s = _lib.stream_handle()
    g = torch.Generator(device="cuda").manual_seed(1)
    copy_bytes = 1 << 30
    src, dst = torch.zeros(copy_bytes // 4, device="cuda"), torch.zeros(copy_bytes // 4, device="cuda")
    t_cp = timed(lambda: call("dl_hbm_copy", ptr(src), ptr(dst), copy_bytes, s), 30, 5)
    rate = 2 * copy_bytes / t_cp / 1e6     # TB/s moved (read + write)
    print("dl_hbm_copy       %8.1f us  %d B read + written: %.2f TB/s" % (t_cp, copy_bytes, rate))
    del src, dst
    blocks, iters = 256 * 16, 4096
    out = torch.zeros(blocks * 256, device="cuda")
    t_f = timed(lambda: call("dl_vfma_probe", ptr(out), out.numel(), blocks, iters, s), 30, 5)
    vf = blocks * 256 * 32.0 * iters / t_f / 1e6
    print("dl_vfma_probe     %8.1f us  %.1f TFLOP/s f32 vector FMA" % (t_f, vf))
    t_m = timed(lambda: call("dl_mfma_f32_probe", ptr(out), out.numel(), blocks, iters, s), 30, 5)
    mf = blocks * 4 * 8 * 2048.0 * iters / t_m / 1e6
    print("dl_mfma_f32_probe %8.1f us  %.1f TFLOP/s v_mfma_f32_16x16x4_f32" % (t_m, mf))
    ld = (13 + F * E + 1 + 15) // 16 * 16
    x0 = torch.randn(B, ld, device="cuda", generator=g) * 0.5
    dz = torch.randn(B, device="cuda", generator=g) / B
    z = torch.zeros(B, device="cuda")
    dx0 = torch.zeros(B, F * E, device="cuda")
    grid = _lib.lib().dl_autoint_grid(B)
    for L, Hn, D in SHAPES:
        n = F * D + sum(4 * (D if l else E) * D for l in range(L))
        prm = torch.randn(n, device="cuda", generator=g) * 0.2
        slab = torch.zeros(grid, n, device="cuda")
        fwd = lambda: call("dl_autoint_fwd", B, F, E, L, Hn, D, ptr(x0), ld, 0, ptr(prm), None, ptr(z), s)
        bwd = lambda: call("dl_autoint_bwd", B, F, E, L, Hn, D, ptr(x0), ld, 0, ptr(prm), ptr(dz), ptr(dx0), F * E, 0,
                           ptr(slab), grid, s)
        bf, bb = B * F * E * 4 + B * 4, 3 * B * F * E * 4 + B * 4
        ff = B * fwd_flops(L, D)
        for name, fn, nbytes, flops in (("dl_autoint_fwd", fwd, bf, ff), ("dl_autoint_bwd", bwd, bb, 3 * ff)):
            t = timed(fn)
            print("F=%d E=%d L=%d Hn=%d D=%d %-14s %9.1f us  %d B: %.1f us at the copy's rate; %.1f GFLOP: %.1f us at "
                  "the f32 matrix rate, %.1f us at the vector FMA rate (%.2f TFLOP/s reached: %.1f%% of the matrix "
                  "rate, %.1f%% of the vector FMA rate)"
                  % (F, E, L, Hn, D, name, t, nbytes, nbytes / rate / 1e6, flops / 1e9, flops / mf / 1e6,
                     flops / vf / 1e6, flops / t / 1e6, 100 * flops / t / 1e6 / mf, 100 * flops / t / 1e6 / vf))
        del slab, prm


def step():
    from deep_learning_amd.engine import CTREngine, ModelSpec
    from deep_learning_amd.synthetic import make_batch
    V = 1_000_000
    bs = [make_batch(B, cate_index_size=V, seed=i) for i in range(4)]
    L, Hn, D = SHAPES[0]
    for on in (0, L, 0, L):
        eng = CTREngine(ModelSpec("dnn_pipeline", C=13, S=26, E=16, cate_index_size=V, hidden=[400, 400, 400],
                                  autoint_layers=on, autoint_heads=Hn, autoint_dim=D), max_batch=B, seed=1, adam="lazy")
        for i in range(4):
            eng.train_step(bs[i % 4], graph=True)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(10):
            eng.train_step(bs[i % 4], graph=True)
        e1.record()
        torch.cuda.synchronize()
        eng.check_error()
        print("dnn_pipeline C2 step, autoint_layers=%d heads=%d dim=%d %9.1f us a step (10 graph steps, host feed "
              "included)" % (on, Hn, D, e0.elapsed_time(e1) * 1e3 / 10))
        del eng


if __name__ == "__main__":
    step() if "--step" in sys.argv else kernels()
