"""The batch-norm kernels (csrc/bn.hip) alone at B = 65,536, D = 400 (a C2 hidden layer, pitch 416),
beside dl_hbm_copy of 1 GiB (bench.py's HBM yardstick) measured in the same run and applied to each
kernel's algorithmic bytes.  Event-timed means; the operands (105 MB a matrix) may partly stay in the
Infinity Cache across these back-to-back launches.

--step: instead, the whole training step of the C2 dnn_pipeline (26 fields, E = 16, hidden 400 x 3,
B = 65,536, lazy tables, hipGraph replay) event-timed with batch_norm off and on, alternating.

Algorithmic bytes (M = 4 B D, one matrix): dl_bn_stats one read (M); dl_bn_fwd training a read and two
writes plus the sign bits (3 M + B D / 8), inference a read and a write (2 M + bits); dl_bn_bwd_sums two
reads (2 M) and the slab; dl_bn_bwd_apply two reads and a write (3 M) and the slab's merge."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deep_learning_amd import _lib  # noqa: E402
from deep_learning_amd._lib import call, ptr  # noqa: E402

B, D, LD, N = 65536, 400, 416, 30


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
    print("dl_hbm_copy      %8.1f us  %d B read + written: %.2f TB/s" % (t_cp, copy_bytes, rate))
    del src, dst
    C = torch.randn(B, LD, device="cuda", generator=g)
    hx = torch.zeros(B, LD, device="cuda")
    dy = torch.randn(B, LD, device="cuda", generator=g) / B
    par = torch.cat([torch.ones(D, device="cuda"), torch.zeros(D, device="cuda")])
    run = torch.stack([torch.zeros(D, device="cuda"), torch.ones(D, device="cuda")])
    stat = torch.zeros(3 * LD, device="cuda")
    sums = torch.zeros(2 * LD, device="cuda")
    ws = torch.zeros(_lib.lib().dl_bn_ws_floats(B, D), device="cuda")
    ldb = 32
    bits = torch.zeros(B, ldb, dtype=torch.int16, device="cuda")
    grid = _lib.lib().dl_bn_grid(B)
    slab = torch.zeros(grid, 2 * D, device="cuda")
    M, nbits, nslab = 4 * B * D, B * ((D + 15) // 16) * 2, grid * 2 * D * 4
    cases = (
        ("dl_bn_stats", M + ws.numel() * 8,
         lambda: call("dl_bn_stats", B, D, ptr(C), LD, 1e-5, 0.1, ptr(stat), ptr(run[0]), ptr(run[1]), None, ptr(ws),
                      ws.numel(), s)),
        ("dl_bn_fwd train", 3 * M + nbits,
         lambda: call("dl_bn_fwd", B, D, ptr(C), LD, ptr(stat), None, None, 1e-5, ptr(par), ptr(hx), LD, ptr(bits), ldb, s)),
        ("dl_bn_fwd infer", 2 * M + nbits,
         lambda: call("dl_bn_fwd", B, D, ptr(C), LD, None, ptr(run[0]), ptr(run[1]), 1e-5, ptr(par), None, 0, ptr(bits),
                      ldb, s)),
        ("dl_bn_bwd_sums", 2 * M + nslab,
         lambda: call("dl_bn_bwd_sums", B, D, ptr(dy), LD, ptr(hx), LD, ptr(slab), grid, s)),
        ("dl_bn_bwd_apply", 3 * M + nslab,
         lambda: call("dl_bn_bwd_apply", B, D, ptr(dy), LD, ptr(hx), LD, ptr(par), ptr(stat), ptr(slab), grid, ptr(sums), s)),
    )
    for name, nbytes, fn in cases:
        t = timed(fn)
        print("%-16s %8.1f us  %d B: %.1f us at the copy's rate, %.2f TB/s reached (%.0f%% of the copy's)"
              % (name, t, nbytes, nbytes / rate / 1e6, nbytes / t / 1e6, 100 * nbytes / t / 1e6 / rate))


def step():
    from deep_learning_amd.engine import CTREngine, ModelSpec
    from deep_learning_amd.synthetic import make_batch
    V = 1_000_000
    bs = [make_batch(B, cate_index_size=V, seed=i) for i in range(4)]
    for bn in (False, True, False, True):
        eng = CTREngine(ModelSpec("dnn_pipeline", C=13, S=26, E=16, cate_index_size=V, hidden=[400, 400, 400],
                                  batch_norm=bn), max_batch=B, seed=1, adam="lazy")
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
        print("dnn_pipeline C2 step, batch_norm=%-5s  %8.1f us a step (20 graph steps, host feed included)"
              % (bn, e0.elapsed_time(e1) * 1e3 / 20))
        del eng


if __name__ == "__main__":
    step() if "--step" in sys.argv else kernels()
