"""Numpy float64 references of the eval metrics of deep_learning_amd/metrics.py (test
infrastructure for test_gauc_cpu.py and test_gpu_gauc.py): GAUC as a plain loop over the groups
with the oracle's tie-aware AUC on each, and the oracle's eps-log-loss with the calibration sums.
"""
import numpy as np

from oracle import ctr_ref as R


def gauc(labels, scores, groups, weighting="size"):
    """(gauc, covered_samples, valid_groups, groups).  A group is valid iff it holds both classes;
    gauc = sum_valid w_g AUC_g / sum_valid w_g with w_g = n_g ("size") or 1 ("uniform"), NaN when
    no group is valid.  Scores are compared as float32 (what the device sorts)."""
    y = np.asarray(labels, np.float64).reshape(-1) > 0.5
    s = np.asarray(scores, np.float32).reshape(-1)
    g = np.asarray(groups, np.int64).reshape(-1)
    order = np.argsort(g, kind="stable")
    ids, start, count = np.unique(g[order], return_index=True, return_counts=True)
    num = den = 0.0
    covered = valid = 0
    for a, n in zip(start, count):
        sel = order[a:a + n]
        yg = y[sel]
        pos = int(yg.sum())
        if pos == 0 or pos == n:
            continue
        w = float(n) if weighting == "size" else 1.0
        num += w * R.auc(yg, s[sel])
        den += w
        covered += int(n)
        valid += 1
    return (num / den if valid else float("nan")), covered, valid, len(ids)


def eval_stats(labels, scores, eps=1e-7):
    """The oracle's log-loss formula (oracle/ctr_ref.py forward: -y log(p + eps) - (1 - y)
    log(1 - p + eps)) in float64 on the float32 scores, and the calibration sums."""
    y = (np.asarray(labels, np.float64).reshape(-1) > 0.5).astype(np.float64)
    p = np.asarray(scores, np.float32).reshape(-1).astype(np.float64)
    per = -y * np.log(p + eps) - (1 - y) * np.log(1 - p + eps)
    n = p.size
    sy = float(y.sum())
    sp = float(p.sum())
    return {"logloss": float(per.sum()) / n, "calibration": sp / sy if sy else float("inf") if sp > 0 else float("nan"),
            "mean_score": sp / n, "positive_rate": sy / n, "n": n}


def case3():
    """The heavy-tailed case of the GAUC tests: 200,003 samples in 3,726 groups, the largest
    beyond one 4,096-element scan tile, scores on a 1/200 grid (many ties)."""
    rng = np.random.default_rng(7)
    n = 200_003
    g = (rng.pareto(1.2, n) * 50).astype(np.int64) % 40000
    s = (np.round(rng.random(n) * 200) / 200 - 0.5).astype(np.float32)
    y = (rng.random(n) < 0.3 + 0.2 * s).astype(np.float32)
    return y, s, g
