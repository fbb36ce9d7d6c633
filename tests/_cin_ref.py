"""Float64 restatement of the Compressed Interaction Network beside the dnn_* tower (ModelSpec.cin_layers;
xDeepFM, Lian et al. 2018, eq. 6-8: direct form, identity activation, no bias, no split-half), for the tests:

    X^0 = the fields [F, E] (single embeddings, then pooled slots), H_0 = F
    X^k[h, e] = sum_{i < H_{k-1}} sum_{j < F} W^k[h, i, j] X^{k-1}[i, e] X^0[j, e]          k = 1 .. L
    z_cin = sum_k sum_h c[off_k + h] sum_e X^k[h, e];   z = tower (+ cross) (+ afm) (+ ccpm) + z_cin
    variables: cin_layer_{k-1} [H_{k-1} F, H_k] (row i F + j), cin_res [sum H_k, 1]; l2 / 2 sum cin_res^2 joins
    the regulariser

* cin_fwd64 / cin_bwd64: the branch alone in numpy, from the closed formulas (float64);
* cin_fwd_bwd32: the same formulas once more as torch float32 einsums on the CPU: the rounding a float32
  evaluation of the fixture shows, for the GPU test's bound at the large shapes;
* torch_branch / torch_fwd_bwd: the branch by torch-CPU float64 autograd;
* forward_backward / train_step: the whole model (tests/_ccpm_ref.py's path, its branch included, with the
  CIN added), one step of oracle.ctr_ref.AdamTF1 on its gradients.

The activation is the identity, so no sign decision can differ between float32 and float64: every sample is
compared.
"""
import math

import numpy as np
import torch

from oracle import ctr_ref as R
from tests import _afm_ref as Af
from tests import _bn_ref as Bn
from tests import _ccpm_ref as Cc
from tests import _pnn_ref as Pn

F32 = np.float32
X = Af.X
MODELS = Af.MODELS

# the GPU test's kernel shapes (F, E, layers)
SHAPES = [(2, 8, (1,)), (3, 8, (2,)), (5, 16, (3, 5)), (26, 16, (16, 16)), (16, 8, (64, 64, 64)), (64, 32, (64,))]


def keys(layers):
    """The variable names in the device vector's order [c | W^1 | W^2 ..]."""
    return ["cin_res"] + ["cin_layer_%d" % k for k in range(len(layers))]


def shapes(F, layers):
    H = (F,) + tuple(layers)
    out = {"cin_res": (sum(layers), 1)}
    for k in range(len(layers)):
        out["cin_layer_%d" % k] = (H[k] * F, H[k + 1])
    return out


def n_params(F, layers):
    return sum(int(np.prod(s)) for s in shapes(F, layers).values())


def n_weights(F, layers):
    return n_params(F, layers) - sum(layers)


def init(F, layers, rng):
    """The engine's initialisation: glorot-uniform layers (fan-in H_{k-1} F, fan-out H_k), cin_res
    ~ N(0, sqrt(2 / (sum H + 1)))."""
    P = {}
    for k, s in shapes(F, layers).items():
        if k == "cin_res":
            P[k] = (rng.standard_normal(s) * math.sqrt(2.0 / (s[0] + 1))).astype(F32)
        else:
            lim = math.sqrt(6.0 / (s[0] + s[1]))
            P[k] = rng.uniform(-lim, lim, s).astype(F32)
    return P


def pack(P, F, layers):
    """The device parameter vector, rounded up to 4 floats."""
    v = np.concatenate([np.asarray(P[k], F32).reshape(-1) for k in keys(layers)])
    assert len(v) == n_params(F, layers)
    return np.concatenate([v, np.zeros(-len(v) % 4, F32)])


def _w(P, k, Hp, F, dtype):
    """cin_layer_k as [H_{k-1}, F, H_k]."""
    a = np.asarray(P["cin_layer_%d" % k], dtype)
    return a.reshape(Hp, F, a.shape[1])


def cin_fwd64(x, P, layers):
    """x [B, F, E] -> z [B] and the maps [X^0, X^1, .., X^L] (each [B, H_k, E])."""
    x = np.asarray(x, np.float64)
    F = x.shape[1]
    c = np.asarray(P["cin_res"], np.float64).reshape(-1)
    maps, z, o = [x], np.zeros(x.shape[0]), 0
    for k, H in enumerate(layers):
        W = _w(P, k, maps[-1].shape[1], F, np.float64)
        maps.append(np.einsum("ijh,bie,bje->bhe", W, maps[-1], x, optimize=True))
        z = z + maps[-1].sum(2) @ c[o:o + H]
        o += H
    return z, maps


def cin_bwd64(x, P, layers, dz):
    """dz [B] -> dx [B, F, E] (the branch's addend to dx0's fields) and the parameter gradients (batch sums)
    as a dict in the variables' shapes."""
    x = np.asarray(x, np.float64)
    dz = np.asarray(dz, np.float64)
    F = x.shape[1]
    _, maps = cin_fwd64(x, P, layers)
    c = np.asarray(P["cin_res"], np.float64).reshape(-1)
    offs = np.concatenate([[0], np.cumsum(layers)])
    G = {"cin_res": np.concatenate([(dz[:, None] * maps[k + 1].sum(2)).sum(0) for k in range(len(layers))])[:, None]}
    dx = np.zeros_like(x)
    g = None
    for k in range(len(layers) - 1, -1, -1):
        D = dz[:, None, None] * c[offs[k]:offs[k + 1]][None, :, None]
        if g is not None:
            D = D + g
        W = _w(P, k, maps[k].shape[1], F, np.float64)
        G["cin_layer_%d" % k] = np.einsum("bhe,bie,bje->ijh", D, maps[k], x, optimize=True).reshape(-1, layers[k])
        dZ = np.einsum("ijh,bhe->bije", W, D, optimize=True)
        g = np.einsum("bije,bje->bie", dZ, x, optimize=True)
        dx += np.einsum("bije,bie->bje", dZ, maps[k], optimize=True)
    return dx + g, G


def cin_fwd_bwd32(x, P, layers, dz):
    """The same formulas as torch float32 einsums on the CPU: z, dx and the gradient vector in the device
    vector's order, as float64 numpy."""
    t = lambda a: torch.tensor(np.asarray(a, F32))
    xt, dzt = t(x), t(dz)
    F = xt.shape[1]
    c = t(P["cin_res"]).reshape(-1)
    offs = np.concatenate([[0], np.cumsum(layers)])
    Ws, maps, z = [], [xt], torch.zeros(xt.shape[0])
    for k, H in enumerate(layers):
        Ws.append(t(P["cin_layer_%d" % k]).reshape(maps[-1].shape[1], F, H))
        maps.append(torch.einsum("ijh,bie,bje->bhe", Ws[-1], maps[-1], xt))
        z = z + maps[-1].sum(2) @ c[offs[k]:offs[k + 1]]
    G = {"cin_res": torch.cat([(dzt[:, None] * maps[k + 1].sum(2)).sum(0) for k in range(len(layers))])}
    dx, g = torch.zeros_like(xt), None
    for k in range(len(layers) - 1, -1, -1):
        D = dzt[:, None, None] * c[offs[k]:offs[k + 1]][None, :, None]
        if g is not None:
            D = D + g
        G["cin_layer_%d" % k] = torch.einsum("bhe,bie,bje->ijh", D, maps[k], xt).reshape(-1)
        dZ = torch.einsum("ijh,bhe->bije", Ws[k], D)
        g = torch.einsum("bije,bje->bie", dZ, xt)
        dx = dx + torch.einsum("bije,bie->bje", dZ, maps[k])
    n = lambda a: a.numpy().astype(np.float64)
    return n(z), n(dx + g), np.concatenate([n(G[k]).reshape(-1) for k in keys(layers)])


def kernel_fixture(B, F, E, layers, seed):
    """fields ~ N(0, 1/2) with sample B // 2 all zeros (padding), W^k ~ N(0, 1 / sqrt(H_{k-1} F)) so that X^k
    stays O(1) through the layers, c ~ N(0, 1), dz ~ N(0, 1) / B."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((B, F, E)) * 0.5).astype(F32)
    x[B // 2] = 0.0
    P = {}
    for k, s in shapes(F, layers).items():
        P[k] = (rng.standard_normal(s) * (1.0 if k == "cin_res" else 1.0 / math.sqrt(s[0]))).astype(F32)
    dz = (rng.standard_normal(B) / B).astype(F32)
    return x, P, dz


# --------------------------------------------------------------------------- the torch side
def torch_branch(fields, Pt, layers):
    """fields [B, F, E] (torch float64) -> z_cin [B]."""
    F = fields.shape[1]
    m, z, o = fields, 0.0, 0
    for k, H in enumerate(layers):
        W = Pt["cin_layer_%d" % k].reshape(m.shape[1], F, H)
        m = torch.einsum("ijh,bie,bje->bhe", W, m, fields)
        z = z + (m.sum(2) @ Pt["cin_res"][o:o + H])[:, 0]
        o += H
    return z


def torch_fwd_bwd(x, P, layers, dz):
    """The branch alone by autograd: z, dx, {key: gradient} (float64 numpy)."""
    t = lambda a: torch.tensor(np.asarray(a, np.float64), dtype=torch.float64)
    xt = t(x).requires_grad_(True)
    Pt = {k: t(v).requires_grad_(True) for k, v in P.items()}
    z = torch_branch(xt, Pt, layers)
    (z * t(dz)).sum().backward()
    return z.detach().numpy(), xt.grad.numpy(), {k: v.grad.numpy() for k, v in Pt.items()}


n_fields = Cc.n_fields


def init_params(cfg, rng, layers=(), filters=(), **kw):
    """tests/_ccpm_ref.py's parameters plus the CIN's."""
    P = Cc.init_params(cfg, rng, filters, **kw)
    if layers:
        P.update(init(n_fields(cfg), layers, rng))
    return P


def forward_backward(cfg, P, batch, layers=(), filters=(), L=0, A=0, pnn=False, bn=False, bi=False, train=True,
                     eps=Bn.EPS, w=None, masks=None, invs=None):
    """tests/_ccpm_ref.py forward_backward with z_cin added to the logit and cin_res to the regulariser
    (layers = (): exactly that one)."""
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
        z = z + torch_branch(fields, Pt, layers)
        reg = reg + (Pt["cin_res"] ** 2).sum()
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
                fields=n(fields))


def train_step(cfg, P, opt, batch, layers=(), filters=(), L=0, A=0, pnn=False, bn=False, bi=False, m=Bn.MOMENTUM,
               **kw):
    """One TF1 Adam step (oracle.ctr_ref.AdamTF1, float32 state) on the float64 gradients, then, with bn,
    torch's running recurrence (stored as f32)."""
    fw = forward_backward(cfg, P, batch, layers, filters, L, A, pnn, bn, bi, True, **kw)
    opt.apply(P, fw["G"])
    if bn:
        B = np.asarray(batch["label"]).size
        for l, (mu, var) in enumerate(fw["stats"]):
            km, kv = Bn.KEY % (l + 1, "running_mean"), Bn.KEY % (l + 1, "running_var")
            rm, rv = Bn.running_update(P[km], P[kv], mu, var, B, m)
            P[km], P[kv] = rm.astype(F32), rv.astype(F32)
    return fw
