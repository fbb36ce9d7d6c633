"""Exact ROC-AUC with ties on the GPU (``dl_auc``, csrc/metrics.hip) — the semantics of
sklearn.metrics.roc_auc_score, which the reference calls on the collected scores
(models/deepfm_pipeline.py:311,344; wdl.py:343-358; deepfm.py:229; dnn.py:147-161).

Scores stay on the device: the eval/predict loops hand their per-batch score tensors to
an :class:`AucAccumulator` and one ``dl_auc`` call sorts and counts them.  Like sklearn,
a label set with a single class raises ``ValueError``.

Beside the pooled AUC: :func:`group_auc` (GAUC, ``dl_gauc`` — each group's own AUC, weighted by
its impressions; the group id is any categorical slot, the user id for one), :func:`eval_stats`
(log-loss and calibration, ``dl_eval_stats``) and :class:`EvalAccumulator`, which collects what
all of them need batch by batch.
"""
import numpy as np
import torch

from . import _lib
from ._lib import call, ptr

_SINGLE_CLASS = "Only one class present in y_true. ROC AUC score is not defined in that case."


def _dev_f32(x):
    if isinstance(x, torch.Tensor):
        return x.detach().to(device="cuda", dtype=torch.float32).reshape(-1).contiguous()
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x, np.float32).reshape(-1))).cuda()


def roc_auc(labels, scores):
    """AUC of scores (host arrays/lists or device tensors) against 0/1 labels."""
    s, y = _dev_f32(scores), _dev_f32(labels)
    if s.numel() != y.numel():
        raise ValueError("labels and scores differ in length")
    n = s.numel()
    if n == 0:
        raise ValueError(_SINGLE_CLASS)
    ws = torch.empty(int(_lib.lib().dl_auc_workspace_bytes(n)), dtype=torch.uint8, device="cuda")
    out = torch.empty(1, dtype=torch.float64, device="cuda")
    call("dl_auc", ptr(s), 1, ptr(y), 1, n, ptr(ws), ws.numel(), ptr(out), _lib.stream_handle())
    v = float(out.item())
    if v != v:
        raise ValueError(_SINGLE_CLASS)
    return v


class AucAccumulator:
    """Collects device score and label tensors batch by batch; ``result()`` is one dl_auc."""

    def __init__(self):
        self.scores, self.labels = [], []

    def add(self, labels, scores):
        self.scores.append(_dev_f32(scores))
        self.labels.append(_dev_f32(labels))

    def result(self):
        if not self.scores:
            raise ValueError(_SINGLE_CLASS)
        return roc_auc(torch.cat(self.labels), torch.cat(self.scores))


_NO_VALID_GROUP = "No group holds both classes. Group AUC is not defined in that case."
_WEIGHTINGS = {"size": 0, "uniform": 1}


def _dev_i64(x):
    if isinstance(x, torch.Tensor):
        return x.detach().to(device="cuda", dtype=torch.int64).reshape(-1)
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x, np.int64).reshape(-1))).cuda()


def _strided_f32(x):
    """A device f32 view and its element stride: a 1-D device f32 tensor is read where it lies."""
    if isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 1 and x.stride(0) > 0:
        return x.detach(), x.stride(0)
    return _dev_f32(x), 1


def group_auc(labels, scores, groups, weighting="size", details=False):
    """GAUC: the mean over groups of each group's own AUC (``roc_auc`` on its samples alone),
    weighted by the group's sample count (``"size"``) or equally (``"uniform"``), over the groups
    that hold both classes.  ``groups`` are integer ids in [0, 2^31).  Host arrays or device
    tensors.  ``details=True`` returns (gauc, {"covered_samples", "valid_groups", "groups"})."""
    v, covered, valid, total = _gauc_call(labels, scores, groups, weighting)
    if v != v:
        raise ValueError(_NO_VALID_GROUP)
    if details:
        return v, {"covered_samples": covered, "valid_groups": valid, "groups": total}
    return v


def _gauc_call(labels, scores, groups, weighting):
    """dl_gauc's four outputs (the GAUC NaN when no group is valid); raises on bad arguments."""
    if weighting not in _WEIGHTINGS:
        raise ValueError("weighting must be 'size' or 'uniform', got %r" % (weighting,))
    (s, ss), (y, ys), g = _strided_f32(scores), _strided_f32(labels), _dev_i64(groups)
    n = s.numel()
    if y.numel() != n or g.numel() != n:
        raise ValueError("labels, scores and groups differ in length")
    if n == 0:
        return float("nan"), 0, 0, 0
    ws = torch.empty(int(_lib.lib().dl_gauc_workspace_bytes(n)), dtype=torch.uint8, device="cuda")
    out = torch.empty(4, dtype=torch.float64, device="cuda")
    call("dl_gauc", ptr(s), ss, ptr(y), ys, ptr(g), g.stride(0) if n > 1 else 1, n, _WEIGHTINGS[weighting], ptr(ws),
         ws.numel(), ptr(out), _lib.stream_handle())
    v, covered, valid, total = out.tolist()
    if total != total:   # every output NaN: the error word (the workspace's first int32) says why
        if int(ws[:4].view(torch.int32).item()) & _lib.STATUS_BAD_ID:
            raise ValueError("group ids must lie in [0, 2**31)")
        raise _lib.DLError("dl_gauc returned no result")
    return v, int(covered), int(valid), int(total)


def eval_stats(labels, scores, eps=1e-7, weights=None):
    """Log-loss (the reference's eps form, in double), calibration (sum of scores / positives),
    mean score, positive rate and n of scores against 0/1 labels.

    weights (per sample, finite and >= 0; ``dl_eval_stats_weighted``): log-loss = sum w l / sum w,
    calibration = sum w p / sum w y, mean score = sum w p / sum w, positive rate = sum w y / sum w.
    This is the population estimate — the statistics of the traffic a down-sampled or
    importance-weighted set stands for — and not the training loss's normaliser (which divides
    by the count of nonzero weights, tf.losses.log_loss's SUM_BY_NONZERO_WEIGHTS).  ``n`` stays the
    sample count; ``weight_sum`` and ``n_nonzero`` are added.  A zero total weight gives NaN
    statistics.  All-ones weights give the unweighted values."""
    (s, ss), (y, ys) = _strided_f32(scores), _strided_f32(labels)
    n = s.numel()
    if y.numel() != n:
        raise ValueError("labels and scores differ in length")
    if n == 0:
        raise ValueError("no samples")
    if weights is not None:
        w, wst = _strided_f32(weights)
        if w.numel() != n:
            raise ValueError("labels, scores and weights differ in length")
        ws = torch.empty(int(_lib.lib().dl_eval_stats_weighted_workspace_bytes(n)) // 8, dtype=torch.float64,
                         device="cuda")
        out = torch.empty(5, dtype=torch.float64, device="cuda")
        call("dl_eval_stats_weighted", ptr(s), ss, ptr(y), ys, ptr(w), wst, n, float(eps), ptr(ws), ws.numel() * 8,
             ptr(out), _lib.stream_handle())
        loss, sp, sy, sw, nz = out.tolist()
        if sw != sw:
            raise ValueError("weights must be finite and >= 0")
        nan = float("nan")
        cal = sp / sy if sy else (float("inf") if sp > 0 else nan)
        return {"logloss": loss / sw if sw else nan, "calibration": cal, "mean_score": sp / sw if sw else nan,
                "positive_rate": sy / sw if sw else nan, "n": n, "weight_sum": sw, "n_nonzero": int(nz)}
    ws = torch.empty(int(_lib.lib().dl_eval_stats_workspace_bytes(n)) // 8, dtype=torch.float64, device="cuda")
    out = torch.empty(4, dtype=torch.float64, device="cuda")
    call("dl_eval_stats", ptr(s), ss, ptr(y), ys, n, float(eps), ptr(ws), ws.numel() * 8, ptr(out),
         _lib.stream_handle())
    loss, sp, sy, cnt = out.tolist()
    cal = sp / sy if sy else (float("inf") if sp > 0 else float("nan"))
    return {"logloss": loss / cnt, "calibration": cal, "mean_score": sp / cnt, "positive_rate": sy / cnt,
            "n": int(cnt)}


class EvalAccumulator(AucAccumulator):
    """An AucAccumulator that also keeps the batches' group ids (when given): ``result()`` is
    still the AUC; ``results()`` adds log-loss, calibration and — with groups — GAUC, each kernel
    called once on the concatenation."""

    def __init__(self, weighting="size"):
        super().__init__()
        self.groups = []
        self.weights = []
        self.weighting = weighting

    def add(self, labels, scores, groups=None, weights=None):
        """weights: per-sample weights of log-loss and calibration (eval_stats), for every batch
        or for none; AUC and GAUC stay unweighted."""
        super().add(labels, scores)
        if (weights is None) != (not self.weights) and len(self.scores) > 1:
            raise ValueError("weights must be given for every batch or for none")
        if weights is not None:
            w = _dev_f32(weights)
            if w.numel() != self.scores[-1].numel():
                raise ValueError("labels, scores and weights differ in length")
            self.weights.append(w)
        if (groups is None) != (not self.groups) and len(self.scores) > 1:
            raise ValueError("groups must be given for every batch or for none")
        if groups is not None:
            g = _dev_i64(groups)
            if g.numel() != self.scores[-1].numel():
                raise ValueError("labels, scores and groups differ in length")
            self.groups.append(g)

    def results(self):
        if not self.scores:
            raise ValueError(_SINGLE_CLASS)
        y, s = torch.cat(self.labels), torch.cat(self.scores)
        st = eval_stats(y, s, weights=torch.cat(self.weights) if self.weights else None)
        out = {"auc": roc_auc(y, s), "logloss": st["logloss"], "calibration": st["calibration"]}
        if self.groups:
            v, d = group_auc(y, s, torch.cat(self.groups), weighting=self.weighting, details=True)
            out.update(gauc=v, gauc_covered=d["covered_samples"], gauc_groups=d["valid_groups"])
        return out


class ShardedAucAccumulator(AucAccumulator):
    """AUC over every rank's scores (row-sharded eval, shard.py): the local device scores and
    labels are all-gathered (padded to the largest rank's count) and dl_auc runs on the global
    concatenation, so every rank gets the single-GPU value of the whole set."""

    def __init__(self, exch):
        super().__init__()
        self.exch = exch

    def result(self):
        import torch.distributed as dist
        ex = self.exch
        s = torch.cat(self.scores) if self.scores else torch.empty(0, device="cuda")
        y = torch.cat(self.labels) if self.labels else torch.empty(0, device="cuda")
        dev = "cpu" if ex.staged else "cuda"
        n = torch.tensor([s.numel()], dtype=torch.int64, device=dev)
        ns = [torch.empty_like(n) for _ in range(ex.world)]
        dist.all_gather(ns, n, group=ex.group)
        counts = [int(c.item()) for c in ns]
        cap = max(counts)
        if cap == 0:
            raise ValueError(_SINGLE_CLASS)
        pad = torch.zeros(2, cap, dtype=torch.float32, device=dev)
        pad[0, : s.numel()] = s.to(dev)
        pad[1, : y.numel()] = y.to(dev)
        parts = [torch.empty_like(pad) for _ in range(ex.world)]
        dist.all_gather(parts, pad, group=ex.group)
        scores = torch.cat([p[0, :c] for p, c in zip(parts, counts)])
        labels = torch.cat([p[1, :c] for p, c in zip(parts, counts)])
        return roc_auc(labels, scores)
