"""Float64 restatement of the dnn_* models with the attentional pairwise interactions beside the
tower (ModelSpec.afm_attention; the pair and attention layers of test_model/AFM.py:63-129 on the
models' own embedded fields), and with the cross network of tests/_cross_ref.py, for the tests:

    fields  e_0 .. e_{F-1} = single embeddings, then pooled slots        (zero row 0, nonzero-mean pooling)
    q_ij    = e_i * e_j  (i < j, i outer);  u_ij = q_ij W + b;  s_ij = h . relu(u_ij)
    a       = softmax_pairs(s);  z_afm = (sum a_ij q_ij) . p
    z       = h_last . deep_res + deep_res_bias (+ x_L . cross_res) + z_afm
    loss    = data term + l2 * 1/2 * (sum deep_res^2 (+ sum cross_res^2))      (nothing on the attention)

* forward_backward: the whole model in torch-CPU float64, differentiated by autograd; at
  afm_attention = 0 it is tests/_cross_ref.py's (and at cross_layers = 0 too, the oracle's);
* train_step: one step of oracle.ctr_ref.AdamTF1 on those gradients;
* afm_fwd64 / afm_bwd64: the branch alone in numpy float64, the closed formulas (the kernels' reference).
"""
import math

import numpy as np
import torch

from oracle import ctr_ref as R
from tests import _cross_ref as X

F32 = np.float32
MODELS = X.MODELS
AFM_KEYS = ("attention_p", "attention_h", "attention_b", "attention_w")


def init_params(cfg, L, A, rng):
    """tests/_cross_ref.py's parameters plus the attention net's (AFM.py:75-85)."""
    P = X.init_params(cfg, L, rng)
    if A:
        E, g = cfg.E, math.sqrt(2.0 / (A + cfg.E))
        P["attention_w"] = (rng.standard_normal((E, A)) * g).astype(F32)
        P["attention_b"] = (rng.standard_normal((1, A)) * g).astype(F32)
        P["attention_h"] = rng.standard_normal((1, A)).astype(F32)
        P["attention_p"] = rng.standard_normal((E, 1)).astype(F32)
    return P


def pairs(F):
    """The reference's pair order: i outer, j inner."""
    i, j = np.triu_indices(F, 1)
    return i, j


def forward_backward(cfg, P, batch, L=0, A=0, w=None, masks=None, invs=None):
    """z, p, loss (data + regulariser), data, and the gradient of every parameter, float64
    (arguments as tests/_cross_ref.py forward_backward; A: attention units, 0 for no branch)."""
    assert cfg.model in MODELS
    t = lambda a: torch.tensor(np.asarray(a, np.float64), dtype=torch.float64)
    E, S, C = cfg.E, cfg.S, cfg.C
    Pt = {k: t(v).requires_grad_(True) for k, v in P.items()}
    lab = t(batch["label"]).reshape(-1)
    B = lab.shape[0]
    cate = torch.tensor(np.asarray(batch["cate_feats"], np.int64))
    V = torch.cat([torch.zeros(1, E, dtype=torch.float64), Pt["feats_emb"][1:]], 0)
    parts = []
    if C:
        parts.append(t(batch["cont_feats"]).reshape(B, C))
    if cfg.V:
        parts.append(t(batch["vector_feats"]).reshape(B, cfg.V))
    single = V[cate[:, :S]]                                            # [B, S, E]
    pooled = [X._pool(V, cate[:, S + a:S + b_]) for (a, b_, *_) in cfg.multi_ranges]
    parts.append(single.reshape(B, S * E))
    parts += pooled
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
            s = xl @ Pt["cross_layer_%d" % l]
            xl = x0 * s + Pt["cross_bias_%d" % l][:, 0] + xl
        z = z + (xl @ Pt["cross_res"])[:, 0]
        reg = reg + (Pt["cross_res"] ** 2).sum()
    if A:
        fields = torch.cat([single] + [p_[:, None, :] for p_ in pooled], 1)      # [B, F, E]
        pi, pj = pairs(fields.shape[1])
        q = fields[:, pi, :] * fields[:, pj, :]                                    # [B, P, E]
        u = q @ Pt["attention_w"] + Pt["attention_b"]                            # [B, P, A]
        s = (torch.relu(u) * Pt["attention_h"]).sum(2)
        a = torch.softmax(s, 1)
        z = z + ((a[:, :, None] * q).sum(1) @ Pt["attention_p"])[:, 0]
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


def train_step(cfg, P, opt, batch, L=0, A=0, **kw):
    """One TF1 Adam step (oracle.ctr_ref.AdamTF1, float32 state) on the float64 gradients."""
    fw = forward_backward(cfg, P, batch, L, A, **kw)
    opt.apply(P, fw["G"])
    return fw


def afm_scores64(x, b, W, h, dtype=np.float64):
    """x [B, F, E] -> q [B, P, E], u [B, P, A], s [B, P] evaluated in `dtype`."""
    x = np.asarray(x, dtype)
    pi, pj = pairs(x.shape[1])
    q = x[:, pi, :] * x[:, pj, :]
    u = (q[:, :, :, None] * np.asarray(W, dtype)[None, None]).sum(2, dtype=dtype) + np.asarray(b, dtype).reshape(-1)
    s = (np.maximum(u, 0) * np.asarray(h, dtype).reshape(-1)).sum(2, dtype=dtype)
    return q, u, s


def afm_fwd64(x, p, h, b, W):
    """x [B, F, E]; p [E]; h, b [A]; W [E, A] -> z_afm [B], stats [B, 2] = {max s, sum exp(s - max)},
    a [B, P], q, u."""
    q, u, s = afm_scores64(x, b, W, h)
    m = s.max(1)
    ex = np.exp(s - m[:, None])
    den = ex.sum(1)
    a = ex / den[:, None]
    z = ((a[:, :, None] * q).sum(1) * np.asarray(p, np.float64).reshape(-1)).sum(1)
    return z, np.stack([m, den], 1), a, q, u


def afm_bwd64(x, p, h, b, W, dz):
    """The issue's backward: returns dx [B, F, E] (the branch's addend to dx0's fields), dp [E],
    dh [A], db [A], dW [E, A]."""
    x, dz = np.asarray(x, np.float64), np.asarray(dz, np.float64)
    p, h, W = (np.asarray(v, np.float64) for v in (p, h, W))
    p, h = p.reshape(-1), h.reshape(-1)
    z, _, a, q, u = afm_fwd64(x, p, h, b, W)
    do = dz[:, None] * p[None, :]                                   # [B, E]
    da = (q * do[:, None, :]).sum(2)                                # [B, P]
    ds = a * (da - (a * da).sum(1, keepdims=True))
    g = ds[:, :, None] * (h[None, None, :] * (u > 0))               # [B, P, A]
    dq = a[:, :, None] * do[:, None, :] + g @ W.T                   # [B, P, E]
    pi, pj = pairs(x.shape[1])
    dx = np.zeros_like(x)
    for k in range(len(pi)):
        dx[:, pi[k]] += dq[:, k] * x[:, pj[k]]
        dx[:, pj[k]] += dq[:, k] * x[:, pi[k]]
    dp = (dz[:, None] * (a[:, :, None] * q).sum(1)).sum(0)
    dh = (ds[:, :, None] * np.maximum(u, 0)).sum((0, 1))
    db = g.sum((0, 1))
    dW = np.einsum("bpe,bpa->ea", q, g)
    return dx, dp, dh, db, dW


def dyadic_fixture(B, F, E, A, seed, h_scale=1.0):
    """The kernels' fixture: x and W random multiples of 1/8 in [-1, 1], b random odd multiples of
    1/1024 in [-1, 1] — every u is an odd multiple of 1/1024, exact in f32 in any summation order, so
    no ReluGrad decision can differ; h, p ~ N(0, 1), dz ~ U(-1, 1) / B."""
    rng = np.random.default_rng(seed)
    x = (rng.integers(-8, 9, size=(B, F, E)) / 8.0).astype(F32)
    W = (rng.integers(-8, 9, size=(E, A)) / 8.0).astype(F32)
    b = ((2 * rng.integers(-512, 512, size=A) + 1) / 1024.0).astype(F32)
    h = (rng.standard_normal(A) * h_scale).astype(F32)
    p = rng.standard_normal(E).astype(F32)
    dz = (rng.uniform(-1, 1, B) / B).astype(F32)
    return x, p, h, b, W, dz


def pack(p, h, b, W):
    """The device parameter vector [p | h | b | W row-major], rounded up to 4 floats."""
    v = np.concatenate([np.asarray(a, F32).reshape(-1) for a in (p, h, b, W)])
    return np.concatenate([v, np.zeros(-len(v) % 4, F32)])
