"""Float64 restatement of the pipeline-style models and wdl with batch normalisation in the deep tower
(ModelSpec.batch_norm; nn.BatchNorm1d of test_model/NFM.py:160-167, 244-252 after every linear_i,
before the activation), and with the cross network and the attentional interactions of
tests/_afm_ref.py on the dnn_* models so the combinations run through one code path, for the tests:

    c_l   = h_{l-1} deep_l + deep_bias_l
    train: mu = mean_b c_l;  var = mean_b (c_l - mu)^2;   eval: mu, var = the running statistics
    h_l   = relu(weight_l (c_l - mu) / sqrt(var + eps) + bias_l)
    running_mean <- (1 - m) running_mean + m mu;  running_var <- (1 - m) running_var + m var B / (B - 1)
    loss  = the model's data term and regulariser (nothing on weight_l, bias_l)

* forward_backward: the whole model in torch-CPU float64, differentiated by autograd; at bn = False it
  is the oracle's ctr_ref.forward / backward (and tests/_afm_ref.py's with L, A);
* train_step: one step of oracle.ctr_ref.AdamTF1 on those gradients, then the running recurrence;
* bn_fwd64 / bn_bwd64 / running_update: the layer alone in numpy float64 (the kernels' reference).
"""
import numpy as np
import torch

from oracle import ctr_ref as R
from tests import _afm_ref as Af

F32 = np.float32
X = Af.X
KEY = "batch_norm_%d.%s"
EPS, MOMENTUM = 1e-5, 0.1


def bn_keys(cfg, running=True):
    parts = ("weight", "bias") + (("running_mean", "running_var") if running else ())
    return [KEY % (l + 1, p) for l in range(len(cfg.hidden)) for p in parts]


def init_params(cfg, L, A, bn, rng, jitter=0.0):
    """The oracle's parameters (+ tests/_afm_ref.py's on the dnn_* models) plus, with bn, torch's
    initial gamma = 1, beta = 0, running_mean = 0, running_var = 1; jitter: gamma and beta moved off
    them (~ N(1, jitter), N(0, jitter)) so a swapped pair would show."""
    P = Af.init_params(cfg, L, A, rng) if cfg.model in Af.MODELS else R.init_params(cfg, rng)
    if bn:
        for l, D in enumerate(cfg.hidden):
            P[KEY % (l + 1, "weight")] = (1.0 + jitter * rng.standard_normal(D)).astype(F32)
            P[KEY % (l + 1, "bias")] = (jitter * rng.standard_normal(D)).astype(F32)
            P[KEY % (l + 1, "running_mean")] = np.zeros(D, F32)
            P[KEY % (l + 1, "running_var")] = np.ones(D, F32)
    return P


def make_batch(name, kw, B, seed):
    """tests/_cross_ref.py's batch (padding ids among the singles, half-empty multi-hot slots) with the
    dense features of every model that has them and wdl's wide ids."""
    b = X.make_batch(name, kw, B, seed)
    rng = np.random.default_rng(seed + 1000)
    if R.FAMILIES[name]["cont"] and "cont_feats" not in b:
        b["cont_feats"] = rng.random((B, kw["C"])).astype(F32)
    if name == "wdl":
        b.pop("vector_feats", None)
        b["wide_feats"] = rng.integers(0, kw["cate_index_size"], size=(B, kw["Fw"])).astype(np.int64)
    return b


def forward_backward(cfg, P, batch, L=0, A=0, bn=False, train=True, eps=EPS, w=None):
    """z, p, loss (data + regulariser), data, the gradient of every parameter (zeros for the running
    statistics) and, per hidden layer, the batch statistics (mu, biased var), float64.  train=False
    normalises by P's running statistics.  w: effective sample weights (sum w l / N_nz), None: the mean."""
    assert cfg.model == "wdl" or (cfg.model in R.FAMILIES and R.FAMILIES[cfg.model]["cont"] != "field"
                                  and cfg.model != "dnn")
    assert not (L or A) or cfg.model in Af.MODELS
    t = lambda a: torch.tensor(np.asarray(a, np.float64), dtype=torch.float64)
    E, S, C = cfg.E, cfg.S, cfg.C
    Pt = {k: t(v).requires_grad_(not k.startswith("batch_norm") or k.endswith((".weight", ".bias")))
          for k, v in P.items()}
    lab = t(batch["label"]).reshape(-1)
    B = lab.shape[0]
    cate = torch.tensor(np.asarray(batch["cate_feats"], np.int64))
    cont = t(batch["cont_feats"]).reshape(B, C) if C else torch.zeros(B, 0, dtype=torch.float64)
    vec = t(batch["vector_feats"]).reshape(B, cfg.V) if cfg.V else torch.zeros(B, 0, dtype=torch.float64)
    fm = R.is_fm(cfg)
    if cfg.model == "wdl":
        V = Pt["weight_mat"]
        x0 = torch.cat([cont, V[cate].reshape(B, S * E)], 1)
    else:
        zr = lambda a: torch.cat([torch.zeros(1, a.shape[1], dtype=torch.float64), a[1:]], 0)
        V = zr(Pt["feats_emb"])
        single = V[cate[:, :S]]
        pooled = [X._pool(V, cate[:, S + a:S + b_]) for (a, b_, *_) in cfg.multi_ranges]
        x0 = torch.cat([cont, vec, single.reshape(B, S * E)] + pooled, 1)
        fields = torch.cat([single] + [p_[:, None, :] for p_ in pooled], 1)
        if fm:
            w1 = zr(Pt["fm_first_order_emb"])
            fam = R.FAMILIES[cfg.model]["cont"]
            Cf = C if R.fm_cont(cfg) else 0
            cidx = torch.arange(Cf)[None, :].repeat(B, 1) + (cfg.cate_index_size if fam == "last" else 0)
            idx = torch.cat([cidx, cate[:, :S] + (C if fam == "first" else 0)], 1)
            val = torch.cat([cont[:, :Cf], torch.ones(B, S, dtype=torch.float64)], 1)
            pf = [X._pool(w1, cate[:, S + a:S + b_]) for (a, b_, *_) in cfg.multi_ranges]
            first = torch.cat([w1[idx][:, :, 0] * val] + pf, 1)
            e = torch.cat([V[idx] * val[:, :, None]] + [p_[:, None, :] for p_ in pooled], 1)
            s = e.sum(1)
            second = 0.5 * (s * s - (e * e).sum(1))
    h = x0
    stats = []
    for i in range(len(cfg.hidden)):
        pre = h @ Pt["deep_%d" % i] + Pt["deep_bias_%d" % i]
        if bn:
            if train:
                mu = pre.mean(0)
                var = ((pre - mu) ** 2).mean(0)
            else:
                mu, var = Pt[KEY % (i + 1, "running_mean")], Pt[KEY % (i + 1, "running_var")]
            stats.append((mu.detach().numpy().copy(), var.detach().numpy().copy()))
            pre = Pt[KEY % (i + 1, "weight")] * (pre - mu) / torch.sqrt(var + eps) + Pt[KEY % (i + 1, "bias")]
        h = torch.relu(pre)
    l2h = lambda a: 0.5 * (a ** 2).sum()
    if fm:
        z = (torch.cat([first, second, h], 1) @ Pt["deep_fm_weight"])[:, 0] + Pt["deep_fm_bias"][0]
        reg = l2h(Pt["deep_fm_weight"])
    elif cfg.model == "wdl":
        wide = torch.tensor(np.asarray(batch["wide_feats"], np.int64))
        Fw, H = wide.shape[1], cfg.hidden[-1]
        ww = Pt["wdl_weights"][:, 0]
        z = ww[wide].sum(1) + (h * ww[Fw:Fw + H]).sum(1) + Pt["wdl_bias"][0]
        reg = l2h(Pt["wdl_weights"]) + sum(l2h(Pt["deep_%d" % i]) for i in range(len(cfg.hidden)))
    else:
        z = (h @ Pt["deep_res"])[:, 0] + Pt["deep_res_bias"][0, 0]
        reg = l2h(Pt["deep_res"])
    if L:
        xl = x0
        for l in range(L):
            xl = x0 * (xl @ Pt["cross_layer_%d" % l]) + Pt["cross_bias_%d" % l][:, 0] + xl
        z = z + (xl @ Pt["cross_res"])[:, 0]
        reg = reg + l2h(Pt["cross_res"])
    if A:
        pi, pj = Af.pairs(fields.shape[1])
        q = fields[:, pi, :] * fields[:, pj, :]
        u = q @ Pt["attention_w"] + Pt["attention_b"]
        a = torch.softmax((torch.relu(u) * Pt["attention_h"]).sum(2), 1)
        z = z + ((a[:, :, None] * q).sum(1) @ Pt["attention_p"])[:, 0]
    p = torch.sigmoid(z)
    le = float(cfg.logloss_eps)
    per = -lab * torch.log(p + le) - (1 - lab) * torch.log(1 - p + le)
    if w is None:
        data = per.mean()
    else:
        w64 = np.asarray(w, np.float64).reshape(-1)
        nz = int(np.count_nonzero(w64))
        data = (t(w64) * per).sum() * (1.0 / nz if nz else 0.0)
    loss = data + cfg.l2 * reg
    loss.backward()
    n = lambda a: a.detach().numpy()
    G = {k: (n(v.grad) if v.grad is not None else np.zeros(v.shape)) for k, v in Pt.items()}
    return dict(z=n(z), p=n(p), loss=float(loss.detach()), data=float(data.detach()), G=G, stats=stats)


def running_update(rm, rv, mu, var, B, m=MOMENTUM):
    """torch's recurrence: the biased batch variance enters the running one unbiased."""
    rm, rv, mu, var = (np.asarray(a, np.float64) for a in (rm, rv, mu, var))
    return (1 - m) * rm + m * mu, (1 - m) * rv + m * var * B / (B - 1)


def train_step(cfg, P, opt, batch, L=0, A=0, bn=True, eps=EPS, m=MOMENTUM, **kw):
    """One TF1 Adam step (oracle.ctr_ref.AdamTF1, float32 state) on the float64 gradients — the
    running statistics get zero gradients and stay — then the running recurrence (stored as f32)."""
    fw = forward_backward(cfg, P, batch, L, A, bn, True, eps, **kw)
    opt.apply(P, fw["G"])
    if bn:
        B = np.asarray(batch["label"]).size
        for l, (mu, var) in enumerate(fw["stats"]):
            km, kv = KEY % (l + 1, "running_mean"), KEY % (l + 1, "running_var")
            rm, rv = running_update(P[km], P[kv], mu, var, B, m)
            P[km], P[kv] = rm.astype(F32), rv.astype(F32)
    return fw


def bn_fwd64(c, gamma, beta, eps=EPS, running=None):
    """c [B, D] -> dict(mu, var (biased), invstd, xhat, y, h); running = (mean, var): eval mode."""
    c, gamma, beta = (np.asarray(a, np.float64) for a in (c, gamma, beta))
    if running is None:
        mu = c.mean(0)
        var = ((c - mu) ** 2).mean(0)
    else:
        mu, var = (np.asarray(a, np.float64) for a in running)
    invstd = 1.0 / np.sqrt(var + eps)
    xhat = (c - mu) * invstd
    y = gamma * xhat + beta
    return dict(mu=mu, var=var, invstd=invstd, xhat=xhat, y=y, h=np.maximum(y, 0))


def bn_bwd64(dy, xhat, gamma, invstd):
    """dy [B, D] = dL/dy -> dc [B, D], dgamma [D], dbeta [D] (training mode)."""
    dy, xhat, gamma, invstd = (np.asarray(a, np.float64) for a in (dy, xhat, gamma, invstd))
    B = dy.shape[0]
    dbeta, dgamma = dy.sum(0), (dy * xhat).sum(0)
    return gamma * invstd * (dy - dbeta / B - xhat * dgamma / B), dgamma, dbeta


def kernel_fixture(B, D, seed, offset=0.0):
    """The kernels' fixture: c ~ N(0, 1) times a per-column scale in [0.25, 4] plus a per-column offset
    in [-2, 2] (+ offset), gamma in [0.5, 1.5] with mixed signs, beta in [-0.5, 0.5], dy ~ N(0, 1) / B,
    running statistics off their initial values."""
    rng = np.random.default_rng(seed)
    scale = rng.uniform(0.25, 4.0, D)
    c = (rng.standard_normal((B, D)) * scale + rng.uniform(-2, 2, D) + offset).astype(F32)
    gamma = (rng.uniform(0.5, 1.5, D) * rng.choice([-1.0, 1.0], D)).astype(F32)
    beta = rng.uniform(-0.5, 0.5, D).astype(F32)
    dy = (rng.standard_normal((B, D)) / B).astype(F32)
    rm = rng.uniform(-1, 1, D).astype(F32)
    rv = rng.uniform(0.5, 2.0, D).astype(F32)
    return c, gamma, beta, dy, rm, rv


def var_f32(c, centred):
    """The biased column variance evaluated in float32 arithmetic: centred (a mean pass, then the mean
    of the squared deviations) or raw (E[c^2] - mu^2) — what the cancellation test must tell apart."""
    c = np.asarray(c, F32)
    B = F32(c.shape[0])
    mu = c.sum(0, dtype=F32) / B
    if centred:
        d = c - mu
        return mu, (d * d).sum(0, dtype=F32) / B
    return mu, (c * c).sum(0, dtype=F32) / B - mu * mu
