"""The wide weights' FTRL kernels beside the Adam forms at the C5 shape (B = 65,536, Fw = 26,
H = 400, 26 M + 400 rows), on the same ids in the same run: dl_wide_ftrl_gather / dl_wide_ftrl_update
against dl_wide_rec_gather / dl_wide_rec_update — launches for a kernel trace
(rocprofv3 --kernel-trace --stats -- python scripts/ftrl_bench.py) and event-timed means.

The Adam records are timed caught up (stamp = the current step: no replay), the state right after
a flush and the cheapest the Adam forms get; the update's gradient is re-formed before every timed
update (dl_wide_seg_grad, not timed) since both updates reset it.  Algorithmic bytes of either form:
one 16-B record read per gathered row, one 16-B record written per updated row.

    python scripts/ftrl_bench.py [rows]
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deep_learning_amd import _lib  # noqa: E402
from deep_learning_amd._lib import call, ptr  # noqa: E402

B, Fw, H, N = 65536, 26, 400, 30
rows = (int(sys.argv[1]) if len(sys.argv) > 1 else 26_000_000) + H
nw = B * Fw
s = _lib.stream_handle()
g = torch.Generator(device="cuda").manual_seed(3)
z = lambda *sh, dt=torch.float32: torch.zeros(*sh, dtype=dt, device="cuda")
ids = torch.randint(0, rows, (nw,), device="cuda", generator=g)
uniq_l, inv = torch.unique(ids, sorted=True, return_inverse=True)
nu = int(uniq_l.numel())
order = torch.argsort(ids, stable=True)
uniq, refs, off = z(nw, dt=torch.int32), order.to(torch.int32), z(nw + 1, dt=torch.int32)
uniq[:nu] = uniq_l.to(torch.int32)
off[1:nu + 1] = torch.cumsum(torch.bincount(inv, minlength=nu), 0).to(torch.int32)
n_uniq = torch.tensor([nu, 0, 0, 0], dtype=torch.int32, device="cuda")
dz = torch.randn(B, device="cuda", generator=g) / B
hist_len = 4096
hist = torch.full((hist_len,), 1e-3, device="cuda")
opt = z(_lib.OPT_LEN)
opt[:8] = torch.tensor([0.9, 0.999, 1e-3, 1e-3, 0.9, 0.999, 1e-8, 5.0])


def records(third, stamp):
    rec = z((rows + 15) // 16 * 16, 4)
    rec[:, 0] = torch.randn(rec.shape[0], device="cuda", generator=g) * 0.01
    rec[:, 2] = third
    rec.view(torch.int32)[:, 3] = stamp
    return rec


rec_a, rec_f = records(1e-6, 5), records(0.1, 0)
wloc, stash, rep = z(Fw + H + nw + 4), z(nw, 4), z(nw)
gloc, dmark, lng = z(Fw + H + nw, dt=torch.int64), z(416, dt=torch.uint8), z(nw + 1, dt=torch.int32)
parts = z(int(_lib.lib().dl_wide_update_blocks(nw, H)))
acc = z(_lib.LOSS_ACC_SLOTS, dt=torch.float64)

gather_a = lambda: call("dl_wide_rec_gather", ptr(rec_a), rows, ptr(uniq), ptr(n_uniq), nw, Fw, H, ptr(hist), hist_len,
                        ptr(opt), 1e-5, 1, ptr(wloc), ptr(stash), ptr(rep), s)
gather_f = lambda: call("dl_wide_ftrl_gather", ptr(rec_f), rows, ptr(uniq), ptr(n_uniq), nw, Fw, H, ptr(opt), ptr(wloc),
                        ptr(stash), s)
grad = lambda: call("dl_wide_seg_grad", ptr(dz), Fw, ptr(refs), ptr(off), ptr(n_uniq), nw, nw, ptr(gloc[Fw + H:]),
                    ptr(lng), ptr(opt), s)
update_a = lambda: call("dl_wide_rec_update", ptr(rec_a), ptr(n_uniq), nw, ptr(stash), ptr(gloc), Fw, H, 1e-5, ptr(hist),
                        hist_len, ptr(opt), ptr(dmark), ptr(parts), ptr(rep), ptr(acc), s)
update_f = lambda: call("dl_wide_ftrl_update", ptr(rec_f), ptr(n_uniq), nw, ptr(stash), ptr(gloc), Fw, H, 0.05, 1e-3, 0.0,
                        ptr(opt), ptr(dmark), s)


def timed(fn, before=None, n=N):
    tot = 0.0
    for i in range(n + 5):
        if before:
            before()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if i >= 5:
            tot += e0.elapsed_time(e1) * 1e3
    return tot / n


print("rows %d  unique wide rows %d of %d references" % (rows, nu, nw))
res = {}
for name, fn, before in (("dl_wide_rec_gather", gather_a, None), ("dl_wide_ftrl_gather", gather_f, None),
                         ("dl_wide_rec_update", update_a, lambda: (gather_a(), grad())),
                         ("dl_wide_ftrl_update", update_f, lambda: (gather_f(), grad()))):
    res[name] = timed(fn, before)
    print("%-20s %7.1f us" % (name, res[name]))
st = int(opt.view(torch.int32)[_lib.OPT_STATUS].item())
print("status %d" % st)
print("ftrl / adam: gather %.2f  update %.2f" % (res["dl_wide_ftrl_gather"] / res["dl_wide_rec_gather"],
                                                  res["dl_wide_ftrl_update"] / res["dl_wide_rec_update"]))
assert st == 0
