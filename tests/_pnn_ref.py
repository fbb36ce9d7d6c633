"""Float64 restatement of the dnn_* models with the inner-product layer of test_model/PNN.py:78-83
in front of the tower (ModelSpec.pnn = "inner"), and with the cross network and the attentional
interactions of tests/_afm_ref.py so one code path serves the combinations, for the tests:

    fields  e_0 .. e_{F-1} = single embeddings, then pooled slots        (zero row 0, nonzero-mean pooling)
    T_i     = sum_f theta[i, f] e_f;   lp_i = sqrt(sum_e T_i[e]^2)       (gradient 0 where T_i = 0)
    h_0     = relu(x0 deep_0 + deep_bias_0 + lp)
    loss    = data term + l2 * 1/2 * (sum deep_res^2 (+ sum cross_res^2))      (nothing on theta)

* forward_backward: the whole model in torch-CPU float64, differentiated by autograd; at pnn = False
  it is tests/_afm_ref.py's;
* train_step: one step of oracle.ctr_ref.AdamTF1 on those gradients;
* pnn_fwd64 / pnn_bwd64: the product term alone in numpy float64, the closed formulas with the
  0-at-zero rule (the kernels' reference).
"""
import numpy as np
import torch

from oracle import ctr_ref as R  # noqa: F401  (the tests reach the oracle through this module)
from tests import _afm_ref as Af

F32 = np.float32
X = Af.X
MODELS = Af.MODELS
KEY = "product-quadratic-inner"


def init_params(cfg, L, A, pnn, rng, scale=0.01):
    """tests/_afm_ref.py's parameters plus theta [D1, F] ~ N(0, scale) (PNN.py:57: 0.01)."""
    P = Af.init_params(cfg, L, A, rng)
    if pnn:
        F = cfg.S + len(cfg.multi_ranges)
        P[KEY] = (rng.standard_normal((cfg.hidden[0], F)) * scale).astype(F32)
    return P


class _Norm(torch.autograd.Function):
    """sqrt(sum_e T^2) over the last axis with the gradient T / lp, 0 where lp == 0."""

    @staticmethod
    def forward(ctx, T):
        lp = torch.sqrt((T * T).sum(-1))
        ctx.save_for_backward(T, lp)
        return lp

    @staticmethod
    def backward(ctx, g):
        T, lp = ctx.saved_tensors
        safe = torch.where(lp > 0, lp, torch.ones_like(lp))
        return torch.where(lp[..., None] > 0, g[..., None] * T / safe[..., None], torch.zeros_like(T))


def forward_backward(cfg, P, batch, L=0, A=0, pnn=False, w=None, masks=None, invs=None):
    """z, p, loss (data + regulariser), data, and the gradient of every parameter, float64
    (arguments as tests/_afm_ref.py forward_backward; pnn: the product term on layer 0)."""
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
    fields = torch.cat([single] + [p_[:, None, :] for p_ in pooled], 1)          # [B, F, E]
    h = x0
    assert masks is None or (masks[0] is None and (not pnn or masks[1] is None))
    lp = None
    for i in range(len(cfg.hidden)):
        pre = h @ Pt["deep_%d" % i] + Pt["deep_bias_%d" % i]
        if i == 0 and pnn:
            lp = _Norm.apply(torch.einsum("if,bfe->bie", Pt[KEY], fields))       # [B, D1]
            pre = pre + lp
        h = torch.relu(pre)
        if i == 0:
            pre0 = pre
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
        pi, pj = Af.pairs(fields.shape[1])
        q = fields[:, pi, :] * fields[:, pj, :]
        u = q @ Pt["attention_w"] + Pt["attention_b"]
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
    return dict(z=n(z), p=n(p), loss=float(loss.detach()), data=float(data.detach()), G=G, x0=n(x0),
                fields=n(fields), pre0=n(pre0), lp=None if lp is None else n(lp))


def train_step(cfg, P, opt, batch, L=0, A=0, pnn=False, **kw):
    """One TF1 Adam step (oracle.ctr_ref.AdamTF1, float32 state) on the float64 gradients."""
    fw = forward_backward(cfg, P, batch, L, A, pnn, **kw)
    opt.apply(P, fw["G"])
    return fw


def pnn_fwd64(x, theta):
    """x [B, F, E], theta [D1, F] -> lp [B, D1], T [B, D1, E]."""
    T = np.einsum("if,bfe->bie", np.asarray(theta, np.float64), np.asarray(x, np.float64))
    return np.sqrt((T * T).sum(2)), T


def pnn_bwd64(x, theta, d):
    """d [B, D1] = dL/d(pre-activation).  Returns dx [B, F, E] (the addend to dx0's fields) and
    dtheta [D1, F]; u = T / lp is 0 where lp == 0."""
    x, theta, d = (np.asarray(v, np.float64) for v in (x, theta, d))
    lp, T = pnn_fwd64(x, theta)
    u = np.where(lp[:, :, None] > 0, T / np.where(lp > 0, lp, 1.0)[:, :, None], 0.0)
    dT = d[:, :, None] * u
    return np.einsum("if,bie->bfe", theta, dT), np.einsum("bie,bfe->if", dT, x)


def kernel_fixture(B, F, E, D1, seed):
    """The kernels' fixture: fields ~ N(0, 1/2) with sample B // 2 all padding (zeros), theta ~ N(0, 1 / sqrt(F))
    (lp ~ sqrt(E) / 2, far above the 1e-2 the tests assert), the first layer's pre-activation c ~ N(-lp, 1)
    shifted so both signs occur, d ~ N(0, 1) / B."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((B, F, E)) * 0.5).astype(F32)
    pad = B // 2 if B > 1 else None          # (B = 1 keeps its one sample live)
    if pad is not None:
        x[pad] = 0.0
    theta = (rng.standard_normal((D1, F)) / np.sqrt(F)).astype(F32)
    lp, _ = pnn_fwd64(x, theta)
    c = (rng.standard_normal((B, D1)) - lp).astype(F32)
    d = (rng.standard_normal((B, D1)) / B).astype(F32)
    return x, theta, c, d, pad
