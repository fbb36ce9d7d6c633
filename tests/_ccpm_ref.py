"""Float64 restatement of the CCPM branch beside the dnn_* tower (ModelSpec.ccpm_filters; the
Conv2D(3x3, same, relu) + MaxPool2D(2x2) stack, Flatten and Dense(1) of test_model/CCPM.py:45-68 on the
models' own embedded fields), for the tests:

    X[h, w] = e_w[h]  (h < E, w < F; fields = single embeddings, then pooled slots), one channel
    u_l[h, w, c] = b_l[c] + sum_{dh, dw} sum_c' K_l[dh+1, dw+1, c', c] a_{l-1}[h+dh, w+dw, c']   (zero outside)
    a_l = maxpool2x2(relu(u_l))  (floor: a trailing odd row / column is dropped)
    z_ccpm = flatten_channels_last(a_{L-1}) . p;   z = tower (+ cross) (+ afm) + z_ccpm
    backward: relu' = 0 at u <= 0; the pool's gradient to the window's first maximum in (row, column) order

* ccpm_fwd / ccpm_bwd: the branch alone in numpy, the dtype a parameter (float64: the kernels' reference;
  float32: the rounding measurement below);
* undecided: the samples whose ReLU signs or pool decisions a float32 evaluation may take differently;
* forward_backward / train_step: the whole model in torch-CPU float64 autograd (tests/_bi_ref.py's, with
  the branch added), one step of oracle.ctr_ref.AdamTF1 on its gradients.

Rounding margin.  Over the GPU test's five shapes (B = 300, fields ~ N(0, 0.1^2), glorot_uniform kernels,
test_ccpm_cpu.py::test_rounding_margin measures it again) the largest |u_32 - u_64| / max |u_l| between
the float32 and float64 restatements measured 2.21e-7 (at (64, 32, (8, 8)); 0.7e-7 to 1.9e-7 at the
others), rounded up to
    U32_REL = 2.5e-7
and the margin below which a sign or a gap counts as undecided is 8 times that (the kernel sums in
another order):
    MARGIN = 2.0e-6
At that margin and the GPU test's seeds the restatement leaves out at most 1.6 % of a case's samples at
the three small shapes, 4 % at (26, 16, (4, 4)) and 19 to 24 % at (64, 32, (8, 8)).
"""
import math

import numpy as np
import torch
import torch.nn.functional as TF

from oracle import ctr_ref as R
from tests import _afm_ref as Af
from tests import _bi_ref as Bi
from tests import _bn_ref as Bn
from tests import _pnn_ref as Pn

F32 = np.float32
X = Af.X
MODELS = Af.MODELS
make_batch = Bn.make_batch
U32_REL = 2.5e-7
MARGIN = 8 * U32_REL

# the GPU test's kernel shapes (F, E, filters)
SHAPES = [(2, 8, (1,)), (3, 8, (2,)), (9, 8, (2, 3, 2)), (26, 16, (4, 4)), (64, 32, (8, 8))]


def dims(F, E, filters):
    """[(H, W, C)] of the input and of every pooled map."""
    out = [(E, F, 1)]
    for c in filters:
        h, w, _ = out[-1]
        out.append((h // 2, w // 2, int(c)))
    return out


def keys(filters):
    """The reference's variable names in the device vector's order [p | K_0 | b_0 | K_1 | b_1 ...]."""
    ks = ["ccpm_out.kernel"]
    for l in range(len(filters)):
        ks += ["ccpm_conv_%d.kernel" % l, "ccpm_conv_%d.bias" % l]
    return ks


def shapes(F, E, filters):
    d = dims(F, E, filters)
    out = {"ccpm_out.kernel": (d[-1][0] * d[-1][1] * d[-1][2], 1)}
    for l in range(len(filters)):
        out["ccpm_conv_%d.kernel" % l] = (3, 3, d[l][2], d[l + 1][2])
        out["ccpm_conv_%d.bias" % l] = (d[l + 1][2],)
    return out


def n_params(F, E, filters):
    return sum(int(np.prod(s)) for s in shapes(F, E, filters).values())


def init(F, E, filters, rng, bias=0.0):
    """Keras' defaults: glorot_uniform kernels, zero biases (bias > 0: N(0, bias^2) ones, for the tests)."""
    P = {}
    for k, s in shapes(F, E, filters).items():
        if k.endswith("bias"):
            P[k] = (rng.standard_normal(s) * bias).astype(F32)
        else:
            rf = s[0] * s[1] if len(s) == 4 else 1
            fan_in, fan_out = (rf * s[2], rf * s[3]) if len(s) == 4 else s
            lim = math.sqrt(6.0 / (fan_in + fan_out))
            P[k] = rng.uniform(-lim, lim, s).astype(F32)
    return P


def pack(P, F, E, filters):
    """The device parameter vector, rounded up to 4 floats."""
    v = np.concatenate([np.asarray(P[k], F32).reshape(-1) for k in keys(filters)])
    assert len(v) == n_params(F, E, filters)
    return np.concatenate([v, np.zeros(-len(v) % 4, F32)])


def unpack(v, F, E, filters):
    out, o = {}, 0
    for k, s in shapes(F, E, filters).items():
        n = int(np.prod(s))
        out[k] = np.asarray(v[o:o + n]).reshape(s).copy()
        o += n
    return out


def _conv(a, K, b):
    """a [B, H, W, C'] -> u [B, H, W, C], 3x3 'same'."""
    B, H, W, _ = a.shape
    pad = np.zeros((B, H + 2, W + 2, a.shape[3]), a.dtype)
    pad[:, 1:H + 1, 1:W + 1] = a
    u = np.zeros((B, H, W, K.shape[3]), a.dtype) + b
    for dh in range(3):
        for dw in range(3):
            u = u + np.einsum("bhwi,io->bhwo", pad[:, dh:dh + H, dw:dw + W], K[dh, dw])
    return u, pad


def _windows(u):
    """u [B, H, W, C] -> [B, H/2, W/2, C, 4], the window's positions in (row, column) order."""
    B, H, W, C = u.shape
    h, w = H // 2, W // 2
    return u[:, :2 * h, :2 * w].reshape(B, h, 2, w, 2, C).transpose(0, 1, 3, 5, 2, 4).reshape(B, h, w, C, 4)


def ccpm_fwd(x, P, filters, dtype=np.float64):
    """x [B, F, E] -> z [B] and, per layer, (a_prev_padded, u, windows of relu(u), argmax, a)."""
    a = np.asarray(x, dtype).transpose(0, 2, 1)[..., None]
    tape = []
    for l in range(len(filters)):
        K = np.asarray(P["ccpm_conv_%d.kernel" % l], dtype)
        b = np.asarray(P["ccpm_conv_%d.bias" % l], dtype).reshape(-1)
        u, pad = _conv(a, K, b)
        win = _windows(np.maximum(u, 0))
        arg = win.argmax(4)                       # numpy's argmax: the first maximum
        a_out = np.take_along_axis(win, arg[..., None], 4)[..., 0]
        tape.append((pad, u, win, arg, a_out))
        a = a_out
    z = a.reshape(a.shape[0], -1) @ np.asarray(P["ccpm_out.kernel"], dtype).reshape(-1)
    return z, tape


def ccpm_bwd(x, P, filters, dz, dtype=np.float64):
    """dz [B] -> dx [B, F, E] (the branch's addend to dx0's fields) and the parameter gradients (batch
    sums) as a dict in the reference's shapes."""
    _, tape = ccpm_fwd(x, P, filters, dtype)
    dz = np.asarray(dz, dtype)
    p = np.asarray(P["ccpm_out.kernel"], dtype).reshape(-1)
    aL = tape[-1][4]
    B = aL.shape[0]
    G = {"ccpm_out.kernel": (dz[:, None] * aL.reshape(B, -1)).sum(0).reshape(-1, 1)}
    da = (dz[:, None] * p[None, :]).reshape(aL.shape)
    for l in range(len(filters) - 1, -1, -1):
        pad, u, win, arg, _ = tape[l]
        K = np.asarray(P["ccpm_conv_%d.kernel" % l], dtype)
        _, H, W, C = u.shape
        h, w = H // 2, W // 2
        dwin = np.zeros(win.shape, dtype)
        np.put_along_axis(dwin, arg[..., None], da[..., None], 4)
        du = np.zeros(u.shape, dtype)
        du[:, :2 * h, :2 * w] = dwin.reshape(B, h, w, C, 2, 2).transpose(0, 1, 4, 2, 5, 3).reshape(B, 2 * h, 2 * w, C)
        du = du * (u > 0)
        dK = np.zeros(K.shape, dtype)
        dpad = np.zeros(pad.shape, dtype)
        for dh in range(3):
            for dw in range(3):
                dK[dh, dw] = np.einsum("bhwi,bhwo->io", pad[:, dh:dh + H, dw:dw + W], du)
                dpad[:, dh:dh + H, dw:dw + W] += np.einsum("bhwo,io->bhwi", du, K[dh, dw])
        G["ccpm_conv_%d.kernel" % l] = dK
        G["ccpm_conv_%d.bias" % l] = du.sum((0, 1, 2))
        da = dpad[:, 1:H + 1, 1:W + 1]
    return da[..., 0].transpose(0, 2, 1), G


def u_rel_error(x, P, filters):
    """max over the layers of max |u_32 - u_64| / max |u_64| (whole batch)."""
    _, t64 = ccpm_fwd(x, P, filters, np.float64)
    _, t32 = ccpm_fwd(x, P, filters, np.float32)
    return max(float(np.abs(a[1].astype(np.float64) - b[1]).max() / np.abs(b[1]).max()) for a, b in zip(t32, t64))


def undecided(x, P, filters, margin=MARGIN, exact_ties_ok=False):
    """[B] bool: in the float64 restatement some |u| of a pooled window lies below margin * max |u_l| (the
    sample's), or some window with a positive maximum has its two largest u closer than that.
    exact_ties_ok: a gap of exactly 0 counts as decided.  Random floats tie exactly only where the window's
    positions see the same patch (a zero field: table row 0, an empty slot), and then they tie in float32
    too and both sides take the first; the engine tests, whose batches hold such fields, use it."""
    _, tape = ccpm_fwd(x, P, filters, np.float64)
    B = tape[0][1].shape[0]
    bad = np.zeros(B, bool)
    for _, u, _, _, _ in tape:
        thr = margin * np.abs(u).reshape(B, -1).max(1)
        w = np.sort(_windows(u), 4)
        bad |= (np.abs(w).reshape(B, -1) < thr[:, None]).any(1)
        gap = (w[..., 3] - w[..., 2]).reshape(B, -1)
        close = (gap < thr[:, None]) & ~((gap == 0) & exact_ties_ok)
        bad |= ((w[..., 3].reshape(B, -1) > 0) & close).any(1)
    return bad


def kernel_fixture(B, F, E, filters, seed, scale=0.1):
    """fields ~ N(0, scale^2) with sample B // 2 all zeros (B > 1), glorot_uniform kernels, biases
    ~ N(0, 0.01^2), dz ~ U(-1, 1) / B."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((B, F, E)) * scale).astype(F32)
    if B > 1:
        x[B // 2] = 0.0
    P = init(F, E, filters, rng, bias=0.01)
    dz = (rng.uniform(-1, 1, B) / B).astype(F32)
    return x, P, dz


def tie_fixture(B, F, E, filters, seed):
    """Dyadic values (x, K multiples of 1/8, b of 1/64): every u is exact in float32 in any summation order,
    so no decision can differ.  Even samples are constant maps, whose interior windows tie at all four
    positions; odd samples repeat every field and every embedding dimension twice."""
    rng = np.random.default_rng(seed)
    x = (rng.integers(-4, 5, size=(B, F, E)) / 8.0).astype(F32)
    x[1::2, 1::2, :] = x[1::2, 0:2 * (F // 2):2, :]
    x[1::2, :, 1::2] = x[1::2, :, 0::2]
    x[0::2] = (rng.integers(1, 5, size=(len(x[0::2]), 1, 1)) / 8.0).astype(F32)
    P = {}
    for k, s in shapes(F, E, filters).items():
        if k.endswith("bias"):
            P[k] = (rng.integers(-2, 3, size=s) / 64.0).astype(F32)
        elif k.endswith("out.kernel"):
            P[k] = rng.standard_normal(s).astype(F32)
        else:
            P[k] = (rng.integers(-2, 5, size=s) / 8.0).astype(F32)
    dz = (rng.uniform(-1, 1, B) / B).astype(F32)
    return x, P, dz


def positive_ties(x, P, filters):
    """Windows with a positive maximum attained more than once, over the batch and the layers."""
    _, tape = ccpm_fwd(x, P, filters)
    n = 0
    for _, u, _, _, _ in tape:
        w = np.sort(_windows(u), 4)
        n += int(((w[..., 3] > 0) & (w[..., 3] == w[..., 2])).sum())
    return n


# --------------------------------------------------------------------------- the torch side
def torch_branch(fields, Pt, filters):
    """fields [B, F, E] (torch float64) -> z_ccpm [B]: F.conv2d(padding=1), relu, F.max_pool2d(2), a dot
    product; the kernels permuted to torch's [C_out, C_in, 3, 3]."""
    m = fields.transpose(1, 2)[:, None]
    for l in range(len(filters)):
        K = Pt["ccpm_conv_%d.kernel" % l].permute(3, 2, 0, 1)
        m = TF.max_pool2d(torch.relu(TF.conv2d(m, K, Pt["ccpm_conv_%d.bias" % l].reshape(-1), padding=1)), 2)
    return (m.permute(0, 2, 3, 1).reshape(m.shape[0], -1) @ Pt["ccpm_out.kernel"])[:, 0]


def torch_fwd_bwd(x, P, filters, dz):
    """The branch alone by autograd: z, dx, {key: gradient} (float64 numpy)."""
    t = lambda a: torch.tensor(np.asarray(a, np.float64), dtype=torch.float64)
    xt = t(x).requires_grad_(True)
    Pt = {k: t(v).requires_grad_(True) for k, v in P.items()}
    z = torch_branch(xt, Pt, filters)
    (z * t(dz)).sum().backward()
    return z.detach().numpy(), xt.grad.numpy(), {k: v.grad.numpy() for k, v in Pt.items()}


def n_fields(cfg):
    return cfg.S + len(cfg.multi_ranges)


def init_params(cfg, rng, filters=(), bias=0.01, **kw):
    """tests/_bi_ref.py's parameters plus the branch's (biases ~ N(0, bias^2) so that they are read)."""
    P = Bi.init_params(cfg, rng, **kw)
    if filters:
        P.update(init(n_fields(cfg), cfg.E, filters, rng, bias=bias))
    return P


def forward_backward(cfg, P, batch, filters=(), L=0, A=0, pnn=False, bn=False, bi=False, train=True, eps=Bn.EPS,
                     w=None, masks=None, invs=None):
    """tests/_bi_ref.py forward_backward with z_ccpm added to the logit (filters = (): exactly that one)."""
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
        z = z + torch_branch(fields, Pt, filters)
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


def train_step(cfg, P, opt, batch, filters=(), L=0, A=0, pnn=False, bn=False, bi=False, m=Bn.MOMENTUM, **kw):
    """One TF1 Adam step (oracle.ctr_ref.AdamTF1, float32 state) on the float64 gradients, then, with bn,
    torch's running recurrence (stored as f32)."""
    fw = forward_backward(cfg, P, batch, filters, L, A, pnn, bn, bi, True, **kw)
    opt.apply(P, fw["G"])
    if bn:
        B = np.asarray(batch["label"]).size
        for l, (mu, var) in enumerate(fw["stats"]):
            km, kv = Bn.KEY % (l + 1, "running_mean"), Bn.KEY % (l + 1, "running_var")
            rm, rv = Bn.running_update(P[km], P[kv], mu, var, B, m)
            P[km], P[kv] = rm.astype(F32), rv.astype(F32)
    return fw
