"""Float64 restatement of the dnn_* models with the Bi-Interaction pooling of test_model/NFM.py:192-197,
226 joined to the tower input (ModelSpec.bi_interaction), and with the cross network, the attentional
interactions, the product layer and batch normalisation of tests/_afm_ref.py, _pnn_ref.py and
_bn_ref.py (their pieces imported, not edited) so one code path serves the combinations, for the tests:

    fields  e_0 .. e_{F-1} = single embeddings, then pooled slots        (zero row 0, nonzero-mean pooling)
    q       = sum_{f<g} e_f * e_g  ( = 1/2 ((sum_f e_f)^2 - sum_f e_f^2) )                         [B, E]
    x0'     = [cont | vector | single | pooled | q];   h_0 = relu(x0' deep_0 + deep_bias_0)
    the cross network, when on, runs on x0' as well; nothing new is trained

* forward_backward: the whole model in torch-CPU float64, differentiated by autograd; at bi = False it
  is the oracle's ctr_ref.forward / backward (and the earlier restatements');
* train_step: one step of oracle.ctr_ref.AdamTF1 on those gradients (+ the running recurrence with bn);
* bi_fwd64 / bi_bwd64: the pooling alone in numpy float64, closed forms (the kernels' reference);
* bi_f32: the float32 evaluations of q (the prefix chain with float-pair sums that the kernel runs, the
  plain one-fma chain, and the subtractive form), for the cancellation and parity tests.
"""
import numpy as np
import torch

from oracle import ctr_ref as R
from tests import _afm_ref as Af
from tests import _bn_ref as Bn
from tests import _pnn_ref as Pn

F32 = np.float32
X = Af.X
MODELS = Af.MODELS
make_batch = Bn.make_batch


def n_fields(cfg):
    return cfg.S + len(cfg.multi_ranges)


def deep_in(cfg, bi):
    return (cfg.S + len(cfg.multi_ranges)) * cfg.E + cfg.C + cfg.V + (cfg.E if bi else 0)


def init_params(cfg, rng, L=0, A=0, pnn=False, bn=False, bi=False, theta_scale=0.01, jitter=0.0):
    """The earlier restatements' parameters; with bi, deep_0 [deep_in + E, hidden[0]] at its glorot scale
    (the q rows last) and, with L, the cross vectors over the wider input."""
    P = Bn.init_params(cfg, L, A, bn, rng, jitter)
    if pnn:
        P[Pn.KEY] = (rng.standard_normal((cfg.hidden[0], n_fields(cfg))) * theta_scale).astype(F32)
    if bi:
        D, H0, H = deep_in(cfg, True), cfg.hidden[0], cfg.hidden[-1]
        P["deep_0"] = (rng.standard_normal((D, H0)) * np.sqrt(2.0 / (D + H0))).astype(F32)
        for k in list(P):
            if k.startswith(("cross_layer_", "cross_bias_")):
                P[k] = (rng.standard_normal((D, 1)) * np.sqrt(2.0 / (D + D))).astype(F32)
            elif k == "cross_res":
                P[k] = (rng.standard_normal((D, 1)) * np.sqrt(2.0 / (D + H + 1))).astype(F32)
    return P


def forward_backward(cfg, P, batch, L=0, A=0, pnn=False, bn=False, bi=False, train=True, eps=Bn.EPS, w=None,
                     masks=None, invs=None):
    """z, p, loss (data + regulariser), data, the gradient of every parameter (zeros for the running
    statistics), the batch statistics per hidden layer (bn), x0', the fields and q, float64.  Arguments as
    the earlier restatements': w the effective sample weights, masks / invs the hidden layers' dropout."""
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
    single = V[cate[:, :S]]                                            # [B, S, E]
    pooled = [X._pool(V, cate[:, S + a:S + b_]) for (a, b_, *_) in cfg.multi_ranges]
    parts.append(single.reshape(B, S * E))
    parts += pooled
    fields = torch.cat([single] + [p_[:, None, :] for p_ in pooled], 1)          # [B, F, E]
    q = None
    if bi:
        s = fields.sum(1)
        q = 0.5 * (s * s - (fields * fields).sum(1))                   # NFM.py:192-197
        parts.append(q)
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
                fields=n(fields), q=None if q is None else n(q))


def train_step(cfg, P, opt, batch, L=0, A=0, pnn=False, bn=False, bi=False, m=Bn.MOMENTUM, **kw):
    """One TF1 Adam step (oracle.ctr_ref.AdamTF1, float32 state) on the float64 gradients, then, with bn,
    torch's running recurrence (stored as f32)."""
    fw = forward_backward(cfg, P, batch, L, A, pnn, bn, bi, True, **kw)
    opt.apply(P, fw["G"])
    if bn:
        B = np.asarray(batch["label"]).size
        for l, (mu, var) in enumerate(fw["stats"]):
            km, kv = Bn.KEY % (l + 1, "running_mean"), Bn.KEY % (l + 1, "running_var")
            rm, rv = Bn.running_update(P[km], P[kv], mu, var, B, m)
            P[km], P[kv] = rm.astype(F32), rv.astype(F32)
    return fw


def bi_fwd64(x):
    """x [B, F, E] -> q [B, E] = sum_f e_f * P_f, P_f = sum_{g<f} e_g, in float64."""
    x = np.asarray(x, np.float64)
    P = np.cumsum(x, 1) - x
    return (x * P).sum(1)


def bi_bwd64(x, dq):
    """dq [B, E] = dL/dq -> de [B, F, E] = dq * (s - e_f), s = sum_g e_g."""
    x, dq = np.asarray(x, np.float64), np.asarray(dq, np.float64)
    return dq[:, None, :] * (x.sum(1, keepdims=True) - x)


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def bi_f32(x, chain):
    """q evaluated in float32 arithmetic: chain = True, the plain prefix chain (q += e_f * P; P += e_f,
    field by field); chain = "pair", the chain the kernel runs, both running sums kept as float pairs
    (the product's error by an fma, emulated through float64, the sums' by two-sum); chain = False, the
    subtractive form 1/2 (s^2 - sum e^2) with both sums accumulated field by field."""
    x = np.asarray(x, F32)
    B, F, E = x.shape
    if chain == "pair":
        z = np.zeros((B, E), F32)
        P, Pl, acc, accl = z, z.copy(), z.copy(), z.copy()
        for f in range(F):
            v = x[:, f]
            p = v * P
            pe = (v.astype(np.float64) * P - p).astype(F32)
            pe = (v.astype(np.float64) * Pl + pe).astype(F32)
            acc, e = _two_sum(acc, p)
            accl = accl + (e + pe)
            P, e = _two_sum(P, v)
            Pl = Pl + e
        return acc + accl
    if chain:
        q, P = np.zeros((B, E), F32), np.zeros((B, E), F32)
        for f in range(F):
            q = q + x[:, f] * P
            P = P + x[:, f]
        return q
    s, ss = np.zeros((B, E), F32), np.zeros((B, E), F32)
    for f in range(F):
        s = s + x[:, f]
        ss = ss + x[:, f] * x[:, f]
    return F32(0.5) * (s * s - ss)


def kernel_fixture(B, F, E, seed):
    """The kernels' fixture: fields ~ N(0, 1/2) with sample B // 2 all padding (zeros; B = 1 keeps its one
    sample live), dq ~ N(0, 1) / B."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((B, F, E)) * 0.5).astype(F32)
    pad = B // 2 if B > 1 else None
    if pad is not None:
        x[pad] = 0.0
    dq = (rng.standard_normal((B, E)) / B).astype(F32)
    return x, dq, pad
