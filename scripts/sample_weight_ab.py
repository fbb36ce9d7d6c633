"""Times the C2 training step (deepfm_pipeline, 13 dense + 26 categorical fields of 1 M ids, E = 16,
MLP [400] * 3, batch 65,536, lazy tables, hipGraph replay) with sample weighting off or on:

    python scripts/sample_weight_ab.py off|on [--tree DIR] [--steps N] [--reps R] [--label NAME]

off: the plain engine.  on: sample_weight=True, pos_weight 2.5, random weights in {0, 0.5, 1, 3}.
--tree DIR imports the package from another checkout (the parent commit's, for the A/B; it knows
only "off").  Eight device-resident batches are cycled; after a warm-up, R runs of N steps are each
timed between two device events, and one JSON line with the runs' ms per step is printed (append
it to profiles/sample_weight_ab/).  With weighting on, dl_weight_norm is also timed alone."""
import argparse
import json
import os
import sys

import torch

ap = argparse.ArgumentParser()
ap.add_argument("mode", choices=["off", "on"])
ap.add_argument("--tree", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
ap.add_argument("--steps", type=int, default=100)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--label", default=None)
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.tree))

from deep_learning_amd import _lib  # noqa: E402
from deep_learning_amd.engine import CTREngine, ModelSpec  # noqa: E402
from deep_learning_amd.synthetic import make_batch_device  # noqa: E402

B, S, VOCAB = 65536, 26, 1_000_000
kw = dict(C=13, V=0, S=S, E=16, cate_index_size=S * VOCAB, hidden=[400, 400, 400])
on = args.mode == "on"
spec = ModelSpec("deepfm_pipeline", **kw, **({"pos_weight": 2.5} if on else {}))
eng = CTREngine(spec, max_batch=B, adam="lazy", **({"sample_weight": True} if on else {}))
batches = [make_batch_device(B, cate_index_size=S * VOCAB, seed=100 + i) for i in range(8)]
if on:
    g = torch.Generator(device="cuda").manual_seed(7)
    choice = torch.tensor([0.0, 0.5, 1.0, 3.0], device="cuda")
    for b in batches:
        b["weight"] = choice[torch.randint(0, 4, (B,), device="cuda", generator=g)].reshape(B, 1)


def steps(n, k0):
    for i in range(n):
        j = (k0 + i) % len(batches)
        eng.train_step(batches[j], graph=True, next_batch=batches[(j + 1) % len(batches)])


steps(40, 0)
torch.cuda.synchronize()
eng.check_error()
ms = []
for r in range(args.reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    steps(args.steps, r * args.steps)
    b.record()
    b.synchronize()
    ms.append(a.elapsed_time(b) / args.steps)
eng.check_error()
out = {"label": args.label or args.mode, "mode": args.mode, "batch": B,
       "steps": args.steps, "ms_per_step": [round(x, 4) for x in ms], "median_ms": round(sorted(ms)[len(ms) // 2], 4),
       "loss": eng.loss(), "device": torch.cuda.get_device_name(0)}
if on:
    s = _lib.stream_handle()
    us = []
    for _ in range(30):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        _lib.call("dl_weight_norm", _lib.ptr(eng.in_weight), _lib.ptr(eng.in_label), B, 2.5, _lib.ptr(eng.w_eff),
                  _lib.ptr(eng.norm), _lib.ptr(eng.err), s)
        b.record()
        b.synchronize()
        us.append(a.elapsed_time(b) * 1e3)
    out["weight_norm_us_median"] = round(sorted(us)[len(us) // 2], 2)
print(json.dumps(out))
