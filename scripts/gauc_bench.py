"""Times dl_gauc beside dl_auc and dl_eval_stats on the same scores, and the numpy per-group loop
(tests/_gauc_ref.py) on the host: python scripts/gauc_bench.py [reps]
Two inputs: the heavy-tailed test case (200,003 samples, 3,726 groups) and 2 M samples in 100 k
groups.  Each device call is warmed, then timed `reps` times between device events in one
process with its workspace allocated beforehand; the median and the spread are printed, and the
bytes the passes move (counted from n, DESIGN.md "Per-group AUC") over the median time."""
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from deep_learning_amd import _lib  # noqa: E402
from deep_learning_amd._lib import call, ptr  # noqa: E402
from tests import _gauc_ref as G  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 30
GAUC_BYTES, AUC_BYTES = 352, 148      # per sample, all passes


def timed(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    ms.sort()
    return ms[len(ms) // 2], ms[0], ms[-1]


def run(name, y, s, g):
    n = len(y)
    L = _lib.lib()
    ty, ts, tg = (torch.from_numpy(a).cuda() for a in (y, s, g))
    out = torch.empty(4, dtype=torch.float64, device="cuda")
    st = _lib.stream_handle()
    ws_g = torch.empty(int(L.dl_gauc_workspace_bytes(n)), dtype=torch.uint8, device="cuda")
    ws_a = torch.empty(int(L.dl_auc_workspace_bytes(n)), dtype=torch.uint8, device="cuda")
    ws_s = torch.empty(int(L.dl_eval_stats_workspace_bytes(n)), dtype=torch.uint8, device="cuda")
    gauc = timed(lambda: call("dl_gauc", ptr(ts), 1, ptr(ty), 1, ptr(tg), 1, n, 0, ptr(ws_g), ws_g.numel(), ptr(out), st))
    v = out.tolist()
    auc = timed(lambda: call("dl_auc", ptr(ts), 1, ptr(ty), 1, n, ptr(ws_a), ws_a.numel(), ptr(out), st))
    stats = timed(lambda: call("dl_eval_stats", ptr(ts), 1, ptr(ty), 1, n, 1e-7, ptr(ws_s), ws_s.numel(), ptr(out), st))
    t0 = time.perf_counter()
    ref = G.gauc(y, s, g)
    host = (time.perf_counter() - t0) * 1e3
    print("%s: n %d, groups %d (valid %d, covered %d), gauc %.6f (numpy %.6f, diff %.1e)" % (
        name, n, int(v[3]), int(v[2]), int(v[1]), v[0], ref[0], abs(v[0] - ref[0])))
    print("  dl_gauc       median %.3f ms (min %.3f, max %.3f)  %.0f GB/s of %d B/sample  workspace %.1f MB" % (
        gauc + (GAUC_BYTES * n / gauc[0] / 1e6, GAUC_BYTES, ws_g.numel() / 1e6)))
    print("  dl_auc        median %.3f ms (min %.3f, max %.3f)  %.0f GB/s of %d B/sample" % (
        auc + (AUC_BYTES * n / auc[0] / 1e6, AUC_BYTES)))
    print("  dl_eval_stats median %.3f ms (min %.3f, max %.3f)" % stats)
    print("  dl_gauc / dl_auc %.2f x; numpy per-group loop %.1f ms (%.0f x dl_gauc)" % (
        gauc[0] / auc[0], host, host / gauc[0]))


y, s, g = G.case3()
run("case3", y, (s + np.float32(0.5)), g)
rng = np.random.default_rng(1)
n = 2_000_000
run("2M", (rng.random(n) < 0.3).astype(np.float32), rng.random(n).astype(np.float32),
    rng.integers(0, 100_000, n).astype(np.int64))
