"""Float64 restatement of Wide & Deep with FTRL-proximal on the wide weights
(ModelSpec.wide_optimizer = "ftrl"), for the tests:

    z_b   = sum_f w[wide_bf] + sum_j w[Fw + j] h_bj + bias          (wdl.py:225-253)
    loss  = data term + l2 * 1/2 * sum_i sum deep_i^2               (wdl.py:272-275; the term on
                                                                     wdl_weights, :270-271, dropped)
    per touched row r (the batch's unique wide ids and the H deep-output rows Fw + j), g the sum
    of the row's references (TF's _apply_sparse_duplicate_indices):
        n' = n + g^2;  sigma = (sqrt(n') - sqrt(n)) / lr;  z' = z + g - sigma w
        w' = |z'| > l1 ? (sign(z') l1 - z') / (sqrt(n') / lr + 2 l2) : 0
    initial state z = 0, n = 0.1; an untouched row does not move.

* forward_backward: the model in torch-CPU float64, differentiated by autograd; with
  wide_l2=True it keeps the reference's L2 term on wdl_weights and is the oracle's wdl
  forward / backward (tests/test_ftrl_cpu.py pins that);
* ftrl_apply: the step above in numpy float64 on the touched rows;
* FtrlRef: the training loop — FTRL state in float64, oracle.ctr_ref.AdamTF1 (float32 state,
  decayed learning rate) for the table, the tower and wdl_bias.
"""
import numpy as np
import torch

from oracle import ctr_ref as R

N0 = 0.1   # initial_accumulator_value
WIDE = "wdl_weights"


def make_batch(kw, B, seed, id_hi=None, hot=None, weight=False):
    """A wdl batch whose wide ids fall in [0, id_hi) (default: every wdl_weights row, so some alias
    the deep-output rows Fw..Fw+H and some repeat inside the batch); hot: an id placed in column 0
    of every sample."""
    rng = np.random.default_rng(seed)
    rows = kw["cate_index_size"] + kw["hidden"][-1]
    b = {"label": (rng.random((B, 1)) < 0.3).astype(np.float32),
         "cont_feats": rng.random((B, kw["C"])).astype(np.float32),
         "cate_feats": rng.integers(0, kw["cate_index_size"], size=(B, kw["S"])).astype(np.int64),
         "wide_feats": rng.integers(0, id_hi or rows, size=(B, kw["Fw"])).astype(np.int64)}
    if hot is not None:
        b["wide_feats"][:, 0] = hot
    if weight:
        b["weight"] = (rng.random(B) * 2.0).astype(np.float32)
        b["weight"][:: 7] = 0.0
    return b


def forward_backward(cfg, P, batch, wide_l2=False, w=None):
    """z, p, loss, data and the gradient of every parameter (float64).  w: effective sample
    weights (sum w l / N_nz, tests/_sample_weight_ref.py), None: the mean."""
    assert cfg.model == "wdl"
    t = lambda a: torch.tensor(np.asarray(a, np.float64), dtype=torch.float64)
    E, S, C = cfg.E, cfg.S, cfg.C
    Pt = {k: t(v).requires_grad_(True) for k, v in P.items()}
    lab = t(batch["label"]).reshape(-1)
    B = lab.shape[0]
    cate = torch.tensor(np.asarray(batch["cate_feats"], np.int64))
    wide = torch.tensor(np.asarray(batch["wide_feats"], np.int64))
    Fw, H = wide.shape[1], cfg.hidden[-1]
    h = torch.cat([t(batch["cont_feats"]).reshape(B, C), Pt["weight_mat"][cate].reshape(B, S * E)], 1)
    reg = 0.0
    for i in range(len(cfg.hidden)):
        h = torch.relu(h @ Pt["deep_%d" % i] + Pt["deep_bias_%d" % i])
        reg = reg + (Pt["deep_%d" % i] ** 2).sum()
    ww = Pt[WIDE][:, 0]
    z = ww[wide].sum(1) + (h * ww[Fw:Fw + H][None, :]).sum(1) + Pt["wdl_bias"][0]
    if wide_l2:
        reg = reg + (ww ** 2).sum()
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
    return dict(z=n(z), p=n(p), loss=float(loss.detach()), data=float(data.detach()), G=G)


def touched_rows(batch, H):
    """The rows one step touches: the batch's unique wide ids and the H deep-output rows."""
    wide = np.asarray(batch["wide_feats"], np.int64)
    Fw = wide.shape[1]
    return np.union1d(np.unique(wide), np.arange(Fw, Fw + H))


def ftrl_apply(w, z, n, g, rows, lr, l1, l2):
    """The FTRL-proximal step on `rows` of the float64 vectors w, z, n (in place); g: the dense
    gradient (duplicates already summed).  Returns the rows' new z (the L1 margin's subject)."""
    r = np.asarray(rows, np.int64)
    gr = g[r]
    n1 = n[r] + gr * gr
    sigma = (np.sqrt(n1) - np.sqrt(n[r])) / lr
    z1 = z[r] + gr - sigma * w[r]
    w[r] = np.where(np.abs(z1) > l1, (np.sign(z1) * l1 - z1) / (np.sqrt(n1) / lr + 2.0 * l2), 0.0)
    z[r], n[r] = z1, n1
    return z1


class FtrlRef:
    """Wide & Deep trained with FTRL on wdl_weights (float64 state) and TF1 Adam on the rest."""

    def __init__(self, cfg, P, lr, l1, l2):
        self.cfg, self.lr, self.l1, self.l2 = cfg, float(lr), float(l1), float(l2)
        self.P = {k: np.array(v, np.float64 if k == WIDE else np.float32) for k, v in P.items()}
        self.adam_P = {k: v for k, v in self.P.items() if k != WIDE}   # the same arrays: updated in place
        self.opt = R.AdamTF1(cfg, self.adam_P)
        rows = self.P[WIDE].shape[0]
        self.z, self.n = np.zeros(rows), np.full(rows, N0)
        self.margin = np.inf     # min | |z'| - l1 | over every (row, step) update so far
        self.ever = np.zeros(rows, bool)

    @property
    def w(self):
        return self.P[WIDE][:, 0]

    def train_step(self, batch, w=None):
        fw = forward_backward(self.cfg, self.P, batch, w=w)
        rows = touched_rows(batch, self.cfg.hidden[-1])
        z1 = ftrl_apply(self.w, self.z, self.n, fw["G"][WIDE][:, 0], rows, self.lr, self.l1, self.l2)
        self.margin = min(self.margin, float(np.abs(np.abs(z1) - self.l1).min()))
        self.ever[rows] = True
        self.opt.apply(self.adam_P, {k: fw["G"][k] for k in self.adam_P})
        return fw

    def predict(self, batch):
        return R.forward(self.cfg, self.P, batch, dtype=np.float64)["p"]
