"""Float64 restatement of the sample-weighted loss (tf.losses.log_loss(label, out, weights=w),
TF 1.x's default reduction SUM_BY_NONZERO_WEIGHTS) for the tests:

    l_b   = -y ln(p + eps) - (1 - y) ln(1 - p + eps)
    w_b   = weight_b * (1 + (pos_weight - 1) * y_b)
    N_nz  = #{b : w_b != 0};  inv_norm = 1 / N_nz (0 when N_nz == 0)
    loss  = sum_b w_b l_b * inv_norm
    dz_b  = (dl_b/dp) * (w_b * inv_norm) * p (1 - p)

and the helpers that drive the oracle (oracle/ctr_ref.py) with it.
"""
import contextlib

import numpy as np

from oracle import ctr_ref as R

F32 = np.float32


def w_eff_f32(weight, label, pos_weight):
    """dl_weight_norm's effective weights, the same two float32 operations: f = 1 + (pw - 1) y,
    w = weight f.  weight None: all ones.  A weight that is negative, NaN or infinite gives 0 (its
    batch is skipped).  Returns (w_eff f32, N_nz int, inv_norm f32, any bad)."""
    y = np.asarray(label, F32).reshape(-1)
    w = np.ones_like(y) if weight is None else np.asarray(weight, F32).reshape(-1)
    with np.errstate(invalid="ignore"):
        ok = (w >= 0) & np.isfinite(w)
        f = (F32(1) + (F32(pos_weight) - F32(1)) * y).astype(F32)
        we = np.where(ok, (np.where(ok, w, F32(0)) * f).astype(F32), F32(0)).astype(F32)
    nz = int(np.count_nonzero(we))
    inv = F32(1.0 / float(nz)) if nz else F32(0)
    return we, nz, inv, bool((~ok).any())


def norm64(w):
    """(N_nz, inv_norm) of effective weights, in float64."""
    nz = int(np.count_nonzero(np.asarray(w)))
    return nz, (1.0 / nz if nz else 0.0)


def per_sample_loss(p, y, eps):
    p, y = np.asarray(p, np.float64), np.asarray(y, np.float64)
    return -y * np.log(p + eps) - (1 - y) * np.log(1 - p + eps)


def loss64(p, y, w, eps=1e-7):
    """The weighted data term: sum w l / N_nz."""
    _, inv = norm64(w)
    return float((np.asarray(w, np.float64) * per_sample_loss(p, y, eps)).sum() * inv)


def dz64(p, y, w, eps=1e-7):
    """d loss / d z per sample."""
    p, y, w = (np.asarray(a, np.float64) for a in (p, y, w))
    _, inv = norm64(w)
    return (-y / (p + eps) + (1 - y) / (1 - p + eps)) * (w * inv) * p * (1 - p)


def head64(feat, w_head, bias, y, w, eps=1e-7):
    """The output layer on features feat [B, n] (any of the head kernels' inputs, as float64):
    z, p, dz, d feat = dz w_head^T, d w_head = feat^T dz, d bias = sum dz, loss."""
    feat, w_head = np.asarray(feat, np.float64), np.asarray(w_head, np.float64)
    z = feat @ w_head + float(bias)
    p = 1.0 / (1.0 + np.exp(-z))
    dz = dz64(p, y, w, eps)
    return dict(z=z, p=p, dz=dz, dfeat=dz[:, None] * w_head[None, :], dw=feat.T @ dz, db=dz.sum(),
                loss=loss64(p, y, w, eps))


@contextlib.contextmanager
def weighted_oracle(w):
    """Inside: the oracle's backward takes its logit gradient from the weighted loss (R.dlogit
    replaced by the formula above in the oracle's own dtype), so R.backward and R.AdamTF1 run the
    weighted step unchanged."""
    w64 = np.asarray(w, np.float64).reshape(-1)
    _, inv = norm64(w64)

    def dlogit(cfg, p, lab, dtype=F32):
        eps = dtype(cfg.logloss_eps)
        scale = (w64 * inv).astype(dtype)
        dp = (-lab / (p + eps) + (1 - lab) / (1 - p + eps)) * scale
        return (dp * p * (1 - p)).astype(dtype)
    orig = R.dlogit
    R.dlogit = dlogit
    try:
        yield
    finally:
        R.dlogit = orig


def train_step(cfg, P, opt, batch, pos_weight=1.0):
    """oracle.ctr_ref.train_step with the weighted loss: returns the forward dict, its "loss" the
    weighted data term plus the regulariser of the pre-update parameters."""
    fw = R.forward(cfg, P, batch)
    w, _, _, _ = w_eff_f32(batch.get("weight"), batch["label"], pos_weight)
    with weighted_oracle(w):
        G, dz = R.backward(cfg, P, batch, fw)
    fw["loss"] = loss64(fw["p"], fw["label"], w, cfg.logloss_eps) + R._reg_loss(cfg, P)
    fw["dz"] = dz
    opt.apply(P, G)
    return fw


def eval_stats(labels, scores, weights, eps=1e-7):
    """metrics.eval_stats(..., weights=) in numpy double."""
    p = np.asarray(scores, np.float32).astype(np.float64).reshape(-1)
    y = np.asarray(labels, np.float32).reshape(-1) > 0.5
    w = np.asarray(weights, np.float32).astype(np.float64).reshape(-1)
    l = np.where(y, -np.log(p + eps), -np.log(1 - p + eps))
    sw, sp, sy = w.sum(), (w * p).sum(), w[y].sum()
    nan = float("nan")
    return {"logloss": (w * l).sum() / sw if sw else nan,
            "calibration": sp / sy if sy else (float("inf") if sp > 0 else nan),
            "mean_score": sp / sw if sw else nan, "positive_rate": sy / sw if sw else nan,
            "n": int(p.size), "weight_sum": float(sw), "n_nonzero": int(np.count_nonzero(w))}
