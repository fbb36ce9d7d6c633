"""Float64 restatement of AutoInt's interacting layers beside the dnn_* tower (ModelSpec.autoint_layers;
Song et al. 2019, eq. 5-8), for the tests:

    X^0 = the fields [F, E] (single embeddings, then pooled slots), D_0 = E, D_l = D, d = D / Hn
    Q, K, V, R = X^{l-1} Wq_l, Wk_l, Wv_l, Wr_l;  per head A_h = softmax_k(Q_h K_h^T) (unscaled), O_h = A_h V_h
    X^l = relu(O + R);   z_autoint = sum_{f, c} w[f D + c] X^L[f, c];   z = tower (+ the other branches) + z_autoint
    variables: autoint_{q,k,v,r}_{l-1} [D_{l-1}, D], autoint_res [F D, 1]; l2 / 2 sum autoint_res^2 joins the
    regulariser

* autoint_fwd64 / autoint_bwd64: the branch alone in numpy, from the closed formulas (float64);
* autoint_fwd_bwd32: the same formulas evaluated in numpy float32 on the CPU, for the GPU test's fallback bound;
* torch_branch / torch_fwd_bwd: the branch by torch-CPU float64 autograd;
* forward_backward / train_step: the whole model (tests/_cin_ref.py's path, every branch of it included, with
  the interacting layers added last in the chained logit), one step of oracle.ctr_ref.AdamTF1.

U's sign decides the ReLU's gradient, so a float32 evaluation may differ from float64 where |U| is tiny:
kernel_fixture keeps only samples whose every |U| is at least MARGIN times the fixture's largest, and the
model restatement reports the smallest and largest |U| it saw.
"""
import math

import numpy as np
import torch

from tests import _afm_ref as Af
from tests import _bn_ref as Bn
from tests import _ccpm_ref as Cc
from tests import _cin_ref as Ci
from tests import _pnn_ref as Pn

F32 = np.float32
X = Af.X
MODELS = Af.MODELS
MARGIN = 1e-5      # the kernels' tolerance, applied to U

# the GPU test's kernel shapes (F, E, Hn, D, L)
SHAPES = [(2, 8, 1, 8, 1), (3, 8, 2, 8, 1), (5, 16, 4, 8, 2), (26, 16, 2, 16, 2), (33, 8, 4, 32, 3), (64, 32, 4, 32, 3)]


def keys(L):
    """The variable names in the device vector's order [w | Wq_1 | Wk_1 | Wv_1 | Wr_1 | Wq_2 ..]."""
    return ["autoint_res"] + ["autoint_%s_%d" % (m, l) for l in range(L) for m in "qkvr"]


def shapes(F, E, L, D):
    out = {"autoint_res": (F * D, 1)}
    for l in range(L):
        for m in "qkvr":
            out["autoint_%s_%d" % (m, l)] = (D if l else E, D)
    return out


def n_params(F, E, L, D):
    return sum(int(np.prod(s)) for s in shapes(F, E, L, D).values())


def init(F, E, L, D, rng):
    """The engine's initialisation: glorot-uniform matrices, autoint_res ~ N(0, sqrt(2 / (F D + 1)))."""
    P = {}
    for k, s in shapes(F, E, L, D).items():
        if k == "autoint_res":
            P[k] = (rng.standard_normal(s) * math.sqrt(2.0 / (s[0] + 1))).astype(F32)
        else:
            lim = math.sqrt(6.0 / (s[0] + s[1]))
            P[k] = rng.uniform(-lim, lim, s).astype(F32)
    return P


def pack(P, F, E, L, D):
    """The device parameter vector (a multiple of 4 floats already)."""
    v = np.concatenate([np.asarray(P[k], F32).reshape(-1) for k in keys(L)])
    assert len(v) == n_params(F, E, L, D) and len(v) % 4 == 0
    return v


def _fwd(x, P, L, Hn, D, dtype, stable=True):
    x = np.asarray(x, dtype)
    B, F, _ = x.shape
    d = D // Hn
    Xl, cache = x, []
    for l in range(L):
        W = [np.asarray(P["autoint_%s_%d" % (m, l)], dtype) for m in "qkvr"]
        Q, K, V, Rr = (Xl @ w for w in W)
        Qh, Kh, Vh = (a.reshape(B, F, Hn, d) for a in (Q, K, V))
        S = np.einsum("bihc,bkhc->bhik", Qh, Kh)
        if stable:
            S = S - S.max(-1, keepdims=True)
        A = np.exp(S)
        A = A / A.sum(-1, keepdims=True)
        O = np.einsum("bhik,bkhc->bihc", A, Vh).reshape(B, F, D)
        U = O + Rr
        cache.append(dict(X=Xl, W=W, Qh=Qh, Kh=Kh, Vh=Vh, A=A, U=U))
        Xl = np.maximum(U, 0)
    w = np.asarray(P["autoint_res"], dtype).reshape(F, D)
    return (Xl * w).sum((1, 2)), Xl, cache


def _bwd(x, P, L, Hn, D, dz, dtype):
    dz = np.asarray(dz, dtype)
    z, XL, cache = _fwd(x, P, L, Hn, D, dtype)
    B, F, _ = XL.shape
    d = D // Hn
    w = np.asarray(P["autoint_res"], dtype).reshape(F, D)
    G = {"autoint_res": (dz[:, None, None] * XL).sum(0).reshape(-1, 1)}
    dX = dz[:, None, None] * w[None]
    for l in range(L - 1, -1, -1):
        c = cache[l]
        dU = dX * (c["U"] > 0)
        dOh = dU.reshape(B, F, Hn, d)
        dV = np.einsum("bhik,bihc->bkhc", c["A"], dOh)
        dA = np.einsum("bihc,bkhc->bhik", dOh, c["Vh"])
        rho = (c["A"] * dA).sum(-1, keepdims=True)
        dS = c["A"] * (dA - rho)
        dQ = np.einsum("bhik,bkhc->bihc", dS, c["Kh"])
        dK = np.einsum("bhik,bihc->bkhc", dS, c["Qh"])
        ds = [a.reshape(B, F, D) for a in (dQ, dK, dV)] + [dU]
        dX = 0
        for m, g, Wm in zip("qkvr", ds, c["W"]):
            G["autoint_%s_%d" % (m, l)] = np.einsum("bfi,bfo->io", c["X"], g)
            dX = dX + g @ Wm.T
    return z, dX, G, cache


def autoint_fwd64(x, P, L, Hn, D, stable=True):
    """x [B, F, E] -> z [B], X^L [B, F, D] and the per-layer cache (U among it)."""
    return _fwd(x, P, L, Hn, D, np.float64, stable)


def autoint_bwd64(x, P, L, Hn, D, dz):
    """dz [B] -> dx [B, F, E] (the branch's addend to dx0's fields) and the parameter gradients (batch sums)."""
    _, dX, G, _ = _bwd(x, P, L, Hn, D, dz, np.float64)
    return dX, G


def autoint_fwd_bwd32(x, P, L, Hn, D, dz):
    """The same formulas in numpy float32 on the CPU: z, dx and the gradient vector in the device vector's
    order, as float64 numpy."""
    z, dX, G, _ = _bwd(x, P, L, Hn, D, dz, np.float32)
    n = lambda a: np.asarray(a, np.float64)
    return n(z), n(dX), np.concatenate([n(G[k]).reshape(-1) for k in keys(L)])


def u_range(cache):
    """Per sample the smallest |U| over every layer, and the largest |U| of all samples."""
    lo = np.min([np.abs(c["U"]).reshape(c["U"].shape[0], -1).min(1) for c in cache], 0)
    return lo, max(float(np.abs(c["U"]).max()) for c in cache)


def kernel_fixture(B, F, E, Hn, D, L, seed, return_acceptance=False, q_scale=1.0):
    """2 B candidate samples x ~ N(0, 1/2), glorot-uniform matrices (Wq_1 times q_scale), w ~ N(0, 1),
    dz ~ N(0, 1) / B; the first B candidates whose every |U| (float64, every layer) is at least MARGIN times
    the candidates' largest |U| are kept, and B must be found."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((2 * B, F, E)) * 0.5).astype(F32)
    P = init(F, E, L, D, rng)
    P["autoint_q_0"] = (P["autoint_q_0"] * q_scale).astype(F32)
    P["autoint_res"] = rng.standard_normal((F * D, 1)).astype(F32)
    dz = (rng.standard_normal(B) / B).astype(F32)
    lo, hi = u_range(autoint_fwd64(x, P, L, Hn, D)[2])
    ok = lo >= MARGIN * hi
    assert ok.sum() >= B, "only %d of %d candidates pass" % (ok.sum(), 2 * B)
    x = np.ascontiguousarray(x[ok][:B])
    return (x, P, dz, float(ok.mean())) if return_acceptance else (x, P, dz)


# --------------------------------------------------------------------------- the torch side
def torch_branch(fields, Pt, L, Hn, D, urange=None):
    """fields [B, F, E] (torch float64) -> z_autoint [B]; urange (a list) receives every layer's |U| extremes."""
    B, F, _ = fields.shape
    d = D // Hn
    Xl = fields
    for l in range(L):
        Q, K, V, Rr = (Xl @ Pt["autoint_%s_%d" % (m, l)] for m in "qkvr")
        Qh, Kh, Vh = (a.reshape(B, F, Hn, d) for a in (Q, K, V))
        A = torch.softmax(torch.einsum("bihc,bkhc->bhik", Qh, Kh), -1)
        U = torch.einsum("bhik,bkhc->bihc", A, Vh).reshape(B, F, D) + Rr
        if urange is not None:
            urange.append((float(U.detach().abs().min()), float(U.detach().abs().max())))
        Xl = torch.relu(U)
    return (Xl.reshape(B, F * D) @ Pt["autoint_res"])[:, 0]


def torch_fwd_bwd(x, P, L, Hn, D, dz):
    """The branch alone by autograd: z, dx, {key: gradient} (float64 numpy)."""
    t = lambda a: torch.tensor(np.asarray(a, np.float64), dtype=torch.float64)
    xt = t(x).requires_grad_(True)
    Pt = {k: t(v).requires_grad_(True) for k, v in P.items()}
    z = torch_branch(xt, Pt, L, Hn, D)
    (z * t(dz)).sum().backward()
    return z.detach().numpy(), xt.grad.numpy(), {k: v.grad.numpy() for k, v in Pt.items()}


n_fields = Cc.n_fields


def init_params(cfg, rng, autoint=None, layers=(), filters=(), **kw):
    """tests/_cin_ref.py's parameters plus the interacting layers' (autoint = (L, Hn, D))."""
    P = Ci.init_params(cfg, rng, layers, filters, **kw)
    if autoint and autoint[0]:
        P.update(init(n_fields(cfg), cfg.E, autoint[0], autoint[2], rng))
    return P


def forward_backward(cfg, P, batch, autoint=None, layers=(), filters=(), L=0, A=0, pnn=False, bn=False, bi=False,
                     train=True, eps=Bn.EPS, w=None, masks=None, invs=None):
    """tests/_cin_ref.py forward_backward with z_autoint added last to the logit and autoint_res to the
    regulariser (autoint None or 0 layers: exactly that one).  Also returns u_min / u_max, the extremes of
    |U| over the layers."""
    if not autoint or not autoint[0]:
        return Ci.forward_backward(cfg, P, batch, layers, filters, L, A, pnn, bn, bi, train, eps, w, masks, invs)
    assert cfg.model in MODELS
    t = lambda a: torch.tensor(np.asarray(a, np.float64), dtype=torch.float64)
    E, S, C = cfg.E, cfg.S, cfg.C
    Pt = {k: t(v).requires_grad_(not k.startswith("batch_norm") or k.endswith((".weight", ".bias")))
          for k, v in P.items()}
    lab = t(batch["label"]).reshape(-1)
    B = lab.shape[0]
    cate = torch.tensor(np.asarray(batch["cate_feats"], np.int64))
    V = torch.cat([torch.zeros(1, E, dtype=torch.float64), Pt["feats_emb"][1:]], 0)
    parts = []
    if C:
        parts.append(t(batch["cont_feats"]).reshape(B, C))
    if cfg.V:
        parts.append(t(batch["vector_feats"]).reshape(B, cfg.V))
    single = V[cate[:, :S]]
    pooled = [X._pool(V, cate[:, S + a:S + b_]) for (a, b_, *_) in cfg.multi_ranges]
    parts.append(single.reshape(B, S * E))
    parts += pooled
    fields = torch.cat([single] + [p_[:, None, :] for p_ in pooled], 1)
    if bi:
        s = fields.sum(1)
        parts.append(0.5 * (s * s - (fields * fields).sum(1)))
    x0 = torch.cat(parts, 1)
    h = x0
    assert masks is None or masks[0] is None
    stats = []
    for i in range(len(cfg.hidden)):
        pre = h @ Pt["deep_%d" % i] + Pt["deep_bias_%d" % i]
        if i == 0 and pnn:
            pre = pre + Pn._Norm.apply(torch.einsum("if,bfe->bie", Pt[Pn.KEY], fields))
        if bn:
            if train:
                mu = pre.mean(0)
                var = ((pre - mu) ** 2).mean(0)
            else:
                mu, var = Pt[Bn.KEY % (i + 1, "running_mean")], Pt[Bn.KEY % (i + 1, "running_var")]
            stats.append((mu.detach().numpy().copy(), var.detach().numpy().copy()))
            pre = Pt[Bn.KEY % (i + 1, "weight")] * (pre - mu) / torch.sqrt(var + eps) + Pt[Bn.KEY % (i + 1, "bias")]
        h = torch.relu(pre)
        if masks is not None and masks[i + 1] is not None:
            h = h * t(masks[i + 1]) * float(invs[i + 1])
    z = (h @ Pt["deep_res"])[:, 0] + Pt["deep_res_bias"][0, 0]
    reg = (Pt["deep_res"] ** 2).sum()
    if L:
        xl = x0
        for l in range(L):
            xl = x0 * (xl @ Pt["cross_layer_%d" % l]) + Pt["cross_bias_%d" % l][:, 0] + xl
        z = z + (xl @ Pt["cross_res"])[:, 0]
        reg = reg + (Pt["cross_res"] ** 2).sum()
    if A:
        pi, pj = Af.pairs(fields.shape[1])
        pq = fields[:, pi, :] * fields[:, pj, :]
        u = pq @ Pt["attention_w"] + Pt["attention_b"]
        a = torch.softmax((torch.relu(u) * Pt["attention_h"]).sum(2), 1)
        z = z + ((a[:, :, None] * pq).sum(1) @ Pt["attention_p"])[:, 0]
    if filters:
        z = z + Cc.torch_branch(fields, Pt, filters)
    if layers:
        z = z + Ci.torch_branch(fields, Pt, layers)
        reg = reg + (Pt["cin_res"] ** 2).sum()
    ur = []
    z = z + torch_branch(fields, Pt, *autoint, urange=ur)
    reg = reg + (Pt["autoint_res"] ** 2).sum()
    p = torch.sigmoid(z)
    le = float(cfg.logloss_eps)
    per = -lab * torch.log(p + le) - (1 - lab) * torch.log(1 - p + le)
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
    return dict(z=n(z), p=n(p), loss=float(loss.detach()), data=float(data.detach()), G=G, stats=stats, x0=n(x0),
                fields=n(fields), u_min=min(u[0] for u in ur), u_max=max(u[1] for u in ur))


def train_step(cfg, P, opt, batch, autoint=None, layers=(), filters=(), L=0, A=0, pnn=False, bn=False, bi=False,
               m=Bn.MOMENTUM, **kw):
    """One TF1 Adam step (oracle.ctr_ref.AdamTF1, float32 state) on the float64 gradients, then, with bn,
    torch's running recurrence (stored as f32)."""
    fw = forward_backward(cfg, P, batch, autoint, layers, filters, L, A, pnn, bn, bi, True, **kw)
    opt.apply(P, fw["G"])
    if bn:
        B = np.asarray(batch["label"]).size
        for l, (mu, var) in enumerate(fw["stats"]):
            km, kv = Bn.KEY % (l + 1, "running_mean"), Bn.KEY % (l + 1, "running_var")
            rm, rv = Bn.running_update(P[km], P[kv], mu, var, B, m)
            P[km], P[kv] = rm.astype(F32), rv.astype(F32)
    return fw
