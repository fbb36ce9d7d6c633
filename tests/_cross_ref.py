"""Float64 restatement of the dnn_* models with a Deep & Cross network beside the tower
(ModelSpec.cross_layers; test_model/DCN.py:73-96 on the models' own deep input), for the tests:

    x0      = [cont | vector | single embeddings | pooled]        (zero row 0, nonzero-mean pooling)
    x_0     = x0;  s_l = x_l . w_l;  x_{l+1} = x0 * s_l + b_l + x_l      (l = 0..L-1)
    z       = h_last . deep_res + deep_res_bias + x_L . cross_res
    loss    = data term + l2 * 1/2 * (sum deep_res^2 + sum cross_res^2)

* forward_backward: the whole model in torch-CPU float64, differentiated by autograd (sample
  weights and hidden-layer dropout masks optional); at cross_layers = 0 it is the oracle's
  dnn_* forward / backward (tests/test_cross_cpu.py pins that);
* train_step: one step of oracle.ctr_ref.AdamTF1 on those gradients;
* cross_fwd64 / cross_bwd64: the cross network alone in numpy float64, the formulas of the issue
  (the kernels' reference).
"""
import math

import numpy as np
import torch

from oracle import ctr_ref as R

F32 = np.float32
MODELS = ("dnn_pipeline", "dnn_cate", "dnn_multi", "dnn_multi_cate")


def cross_keys(L):
    return ["cross_res"] + ["cross_layer_%d" % l for l in range(L)] + ["cross_bias_%d" % l for l in range(L)]


def init_params(cfg, L, rng):
    """The oracle's parameters plus the cross network's (DCN.py:75-79, :90-93)."""
    P = R.init_params(cfg, rng)
    D, H = R.deep_in(cfg), cfg.hidden[-1]
    g = math.sqrt(2.0 / (D + D))
    for l in range(L):
        P["cross_layer_%d" % l] = (rng.standard_normal((D, 1)) * g).astype(F32)
        P["cross_bias_%d" % l] = (rng.standard_normal((D, 1)) * g).astype(F32)
    if L:
        P["cross_res"] = (rng.standard_normal((D, 1)) * math.sqrt(2.0 / (D + H + 1))).astype(F32)
    return P


def make_batch(name, kw, B, seed):
    """A batch with padding ids (row 0) among the singles, half-empty multi-hot slots and one
    sample whose slots are all padding (count 0)."""
    rng = np.random.default_rng(seed)
    W = sum(e - s for s, e, _ in kw.get("multi_ranges", []))
    cate = rng.integers(1, kw["cate_index_size"], size=(B, kw["S"] + W))
    cate[0, :2] = [0, 1]
    if W:
        multi = cate[:, kw["S"]:]
        multi[rng.random((B, W)) < 0.5] = 0
        multi[1 % B] = 0
    b = {"label": (rng.random((B, 1)) < 0.3).astype(np.float32), "cate_feats": cate.astype(np.int64)}
    if name in ("dnn_pipeline", "dnn_multi"):
        b["cont_feats"] = rng.random((B, kw["C"])).astype(np.float32)
    if kw.get("V"):
        b["vector_feats"] = rng.standard_normal((B, kw["V"])).astype(np.float32)
    return b


def _pool(V, ids):
    """deepfm_multi_cate.py:73-78: sum over the slot / count of rows whose element sum is nonzero."""
    emb = V[ids]                                                   # [B, W, E]
    cnt = (emb.sum(2) != 0).sum(1, keepdim=True).to(emb.dtype).detach()
    s = emb.sum(1)
    return torch.where(cnt > 0, s / torch.where(cnt > 0, cnt, torch.ones_like(cnt)), torch.zeros_like(s))


def forward_backward(cfg, P, batch, L, w=None, masks=None, invs=None):
    """z, p, loss (data + regulariser), data, and the gradient of every parameter, float64.
    w: effective sample weights (tests/_sample_weight_ref.py: sum w l / N_nz), None: the mean.
    masks / invs: hidden-layer dropout, entry i + 1 applied to layer i's output (entry 0, the tower
    input's, must be None: the cross network refuses input dropout)."""
    assert cfg.model in MODELS
    t = lambda a: torch.tensor(np.asarray(a, np.float64), dtype=torch.float64)
    E, S, C = cfg.E, cfg.S, cfg.C
    Pt = {k: t(v).requires_grad_(True) for k, v in P.items()}
    lab = t(batch["label"]).reshape(-1)
    B = lab.shape[0]
    cate = torch.tensor(np.asarray(batch["cate_feats"], np.int64))
    V = torch.cat([torch.zeros(1, E, dtype=torch.float64), Pt["feats_emb"][1:]], 0)     # dnn_pipeline.py zero row 0
    parts = []
    if C:
        parts.append(t(batch["cont_feats"]).reshape(B, C))
    if cfg.V:
        parts.append(t(batch["vector_feats"]).reshape(B, cfg.V))
    parts.append(V[cate[:, :S]].reshape(B, S * E))
    for (a, b_, *_) in cfg.multi_ranges:
        parts.append(_pool(V, cate[:, S + a:S + b_]))
    x0 = torch.cat(parts, 1)
    h = x0
    assert masks is None or masks[0] is None
    for i in range(len(cfg.hidden)):
        h = torch.relu(h @ Pt["deep_%d" % i] + Pt["deep_bias_%d" % i])
        if masks is not None and masks[i + 1] is not None:
            h = h * t(masks[i + 1]) * float(invs[i + 1])
    z = (h @ Pt["deep_res"])[:, 0] + Pt["deep_res_bias"][0, 0]
    reg = (Pt["deep_res"] ** 2).sum()
    if L:
        xl = x0
        for l in range(L):
            s = xl @ Pt["cross_layer_%d" % l]                      # [B, 1]
            xl = x0 * s + Pt["cross_bias_%d" % l][:, 0] + xl
        z = z + (xl @ Pt["cross_res"])[:, 0]
        reg = reg + (Pt["cross_res"] ** 2).sum()
    p = torch.sigmoid(z)
    eps = float(cfg.logloss_eps)
    per = -lab * torch.log(p + eps) - (1 - lab) * torch.log(1 - p + eps)
    if w is None:
        data = per.mean()
    else:
        w64 = np.asarray(w, np.float64).reshape(-1)
        nz = int(np.count_nonzero(w64))
        data = (t(w64) * per).sum() * (1.0 / nz if nz else 0.0)
    loss = data + cfg.l2 * 0.5 * reg
    loss.backward()
    n = lambda a: a.detach().numpy()
    G = {k: (n(v.grad) if v.grad is not None else np.zeros(v.shape)) for k, v in Pt.items()}
    return dict(z=n(z), p=n(p), loss=float(loss.detach()), data=float(data.detach()), G=G, x0=n(x0))


def train_step(cfg, P, opt, batch, L, **kw):
    """One TF1 Adam step (oracle.ctr_ref.AdamTF1, float32 state) on the float64 gradients."""
    fw = forward_backward(cfg, P, batch, L, **kw)
    opt.apply(P, fw["G"])
    return fw


def cross_fwd64(x0, c, w, b):
    """x0 [B, D]; c [D]; w, b [L, D] -> s [B, L], z_cross [B], xs (x_0 .. x_L)."""
    x0 = np.asarray(x0, np.float64)
    xs = [x0]
    s = np.zeros((x0.shape[0], len(w)))
    for l in range(len(w)):
        s[:, l] = xs[l] @ np.asarray(w[l], np.float64)
        xs.append(x0 * s[:, l:l + 1] + np.asarray(b[l], np.float64) + xs[l])
    return s, xs[-1] @ np.asarray(c, np.float64), xs


def cross_bwd64(x0, c, w, b, dz):
    """The issue's backward: returns ddx0 [B, D] (the cross network's share of dx0), dc [D],
    dw [L, D], db [L, D]."""
    x0, dz = np.asarray(x0, np.float64), np.asarray(dz, np.float64)
    s, _, xs = cross_fwd64(x0, c, w, b)
    L = len(w)
    g = dz[:, None] * np.asarray(c, np.float64)[None, :]
    dc = xs[L].T @ dz
    dw, db, dx = np.zeros((L, x0.shape[1])), np.zeros((L, x0.shape[1])), np.zeros_like(x0)
    for l in reversed(range(L)):
        tl = (g * x0).sum(1)
        dw[l] = (tl[:, None] * xs[l]).sum(0)
        db[l] = g.sum(0)
        dx += g * s[:, l:l + 1]
        g = g + tl[:, None] * np.asarray(w[l], np.float64)[None, :]
    return dx + g, dc, dw, db
