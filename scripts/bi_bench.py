"""The Bi-Interaction kernels (csrc/bi.hip) alone at B = 65,536, F = 26, E = 16 (the C2 fields; x0 pitch
448, dx0 pitch 432, q and dq inside those matrices as in the engine), beside dl_hbm_copy of 1 GiB
(bench.py's HBM yardstick) measured in the same run and applied to each kernel's algorithmic bytes.
Event-timed means of 30 launches; the operands (117 MB of x0, 113 MB of dx0) fit the 256 MB Infinity
Cache, so a relaunched kernel may read part of them from there and exceed the copy's rate.

--step: instead, the whole training step of the C2 dnn_pipeline (26 fields, E = 16, hidden 400 x 3,
B = 65,536, lazy tables, hipGraph replay) event-timed with bi_interaction off, off without the first
layer's fused row gather (DLAMD_FUSED_GATHER=0: the form bi_interaction gives up) and on, alternating;
on - off splits into (off unfused - off) = the lost fused form and (on - off unfused) = the two kernels
plus the wider layer 0.

Algorithmic bytes: dl_bi_fwd reads the fields and writes q, 4 B (F E + E); dl_bi_bwd reads the fields and
dq and reads and writes dx0's field columns, 4 B (3 F E + E) (its second read of the fields is not
counted: it is meant to hit cache)."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deep_learning_amd import _lib  # noqa: E402
from deep_learning_amd._lib import call, ptr  # noqa: E402

B, F, E, LD, DX_LD, N = 65536, 26, 16, 448, 432, 30


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
    x0 = torch.randn(B, LD, device="cuda", generator=g) * 0.5
    dx0 = torch.randn(B, DX_LD, device="cuda", generator=g) / B
    cases = (
        ("dl_bi_fwd", 4 * B * (F * E + E),
         lambda: call("dl_bi_fwd", B, F, E, ptr(x0), LD, 0, ptr(x0), LD, F * E, s)),
        ("dl_bi_bwd", 4 * B * (3 * F * E + E),
         lambda: call("dl_bi_bwd", B, F, E, ptr(x0), LD, 0, ptr(dx0), DX_LD, F * E, ptr(dx0), DX_LD, 0, s)),
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
    arms = (("off", False, "1"), ("off unfused", False, "0"), ("on", True, "1"))
    for tag, bi, fused in arms + arms:
        os.environ["DLAMD_FUSED_GATHER"] = fused
        eng = CTREngine(ModelSpec("dnn_pipeline", C=13, S=26, E=16, cate_index_size=V, hidden=[400, 400, 400],
                                  bi_interaction=bi), max_batch=B, seed=1, adam="lazy")
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
        print("dnn_pipeline C2 step, bi_interaction %-12s %8.1f us a step (20 graph steps, host feed included)"
              % (tag, e0.elapsed_time(e1) * 1e3 / 20))
        del eng
    os.environ.pop("DLAMD_FUSED_GATHER", None)


if __name__ == "__main__":
    step() if "--step" in sys.argv else kernels()
