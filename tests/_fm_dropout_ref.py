"""Test-side restatements for the FM part's dropout (include/dlamd.h "Dropout", layers
DL_DROP_LAYER_FM1 / FM2), written from the reference models' math and the header's words, not
from the kernels:

* fm_masks / pack_keep: the two masks in numpy (tests/_dropout_ref.py keep_mask) and the bit
  layout dl_head_fwd_bwd_fmdrop stores them in;
* deepfm_fp64: deepfm_pipeline / deepfm_multi_cate (embedding -> FM first and second order,
  nonzero-mean pooled slots, tower -> head -> eps-log-loss) in float64 torch autograd with
  explicit FM masks, the reference the engine's gradients are compared against.
"""
import numpy as np

from oracle import ctr_ref as R
from tests import _dropout_ref as D

LAYER_FM1, LAYER_FM2 = 1 << 16, (1 << 16) + 1


def fm_masks(seed, step, B, F, E, keeps):
    """bool [B][F] (first order: col = FM column) and [B][E] (second order: col = dim).  A keep
    of exactly 1 keeps everything (no threshold compare is made)."""
    one = lambda layer, n, k: np.ones((B, n), bool) if k == 1.0 else D.keep_mask(seed, step, layer, B, n, k)
    return one(LAYER_FM1, F, keeps[0]), one(LAYER_FM2, E, keeps[1])


def pack_keep(m1, m2):
    """uint64 [B][2]: bit c of word k is FM column 64 k + c of [first order | second order];
    columns past F + E are 0."""
    m = np.concatenate([m1, m2], 1)
    B, n = m.shape
    assert n <= 128
    bits = np.zeros((B, 128), np.uint64)
    bits[:, :n] = m
    w = np.uint64(1) << np.arange(64, dtype=np.uint64)
    return np.stack([(bits[:, :64] * w).sum(1, dtype=np.uint64), (bits[:, 64:] * w).sum(1, dtype=np.uint64)], 1)


def deepfm_fp64(cfg, P, batch, m1, m2, inv1, inv2):
    """deepfm_pipeline (deepfm_pipeline.py:83-183) / deepfm_multi_cate (deepfm_multi_cate.py:71-169)
    in float64 autograd; first_order * m1 * inv1 and second_order * m2 * inv2 before the output
    layer (tf.nn.dropout, deepfm_pipeline.py:98,110).  Returns the logits z, the loss (with its
    L2 term), the gradient of every parameter (reference keys) and dx0 = d loss / d (tower input)
    in the reference's column order [cont, vector, single cate, pooled]."""
    import torch
    f64 = torch.float64
    t = lambda a: torch.tensor(np.asarray(a, np.float64), dtype=f64)
    assert cfg.model in ("deepfm_pipeline", "deepfm_multi_cate")
    S, E, C = cfg.S, cfg.E, cfg.C
    Pt = {k: t(v).requires_grad_(True) for k, v in P.items()}
    lab = t(batch["label"]).reshape(-1)
    B = lab.shape[0]
    cont = t(batch["cont_feats"]) if C else torch.zeros(B, 0, dtype=f64)
    vec = batch.get("vector_feats")
    vec = torch.zeros(B, 0, dtype=f64) if vec is None else t(vec)
    cate = torch.tensor(np.asarray(batch["cate_feats"], np.int64))
    single, multi = cate[:, :S], cate[:, S:]
    zero_row = lambda T: torch.cat([torch.zeros(1, T.shape[1], dtype=f64), T[1:]], 0)      # :83-86
    V, w1 = zero_row(Pt["feats_emb"]), zero_row(Pt["fm_first_order_emb"])

    def nonzero_mean(emb):      # deepfm_multi_cate.py:73-78, emb [B][L][n]
        cnt = (emb.sum(2) != 0).sum(1, keepdim=True).to(f64)
        return torch.where(cnt > 0, emb.sum(1) / torch.where(cnt > 0, cnt, torch.ones_like(cnt)),
                           torch.zeros_like(emb.sum(1)))
    pooled = [nonzero_mean(V[multi[:, a:b]]) for a, b, *_ in cfg.multi_ranges]
    pooled_first = [nonzero_mean(w1[multi[:, a:b]]) for a, b, *_ in cfg.multi_ranges]
    M = len(pooled)
    Cf = C if R.fm_cont(cfg) else 0
    cate_off = C if R.FAMILIES[cfg.model]["cont"] == "first" else 0                         # :89
    idx = torch.cat([torch.arange(Cf).repeat(B, 1), single + cate_off], 1)
    val = torch.cat([cont[:, :Cf], torch.ones(B, S, dtype=f64)], 1)
    first = torch.cat([w1[idx][:, :, 0] * val] + pooled_first, 1)                           # :95-97
    e = torch.cat([V[idx] * val[:, :, None]] + [p[:, None, :] for p in pooled], 1)          # :102-104
    s = e.sum(1)
    second = 0.5 * (s * s - (e * e).sum(1))                                                 # :105-109
    x0 = torch.cat([cont, vec, V[single].reshape(B, S * E)] + pooled, 1)                    # :120-123
    x0.retain_grad()
    h = x0
    for i in range(len(cfg.hidden)):
        h = torch.relu(h @ Pt["deep_%d" % i] + Pt["deep_bias_%d" % i])
    feats = torch.cat([first * t(m1) * float(inv1), second * t(m2) * float(inv2), h], 1)    # :98,110,157
    z = (feats @ Pt["deep_fm_weight"])[:, 0] + Pt["deep_fm_bias"][0]
    p = torch.sigmoid(z)
    eps = float(cfg.logloss_eps)
    per = -lab * torch.log(p + eps) - (1 - lab) * torch.log(1 - p + eps)
    loss = per.mean() + cfg.l2 * 0.5 * (Pt["deep_fm_weight"] ** 2).sum()
    loss.backward()
    n = lambda a: a.detach().numpy()
    zero = lambda v: np.zeros(tuple(v.shape))
    return dict(z=n(z), loss=float(loss.detach()), dx0=n(x0.grad), M=M,
                G={k: (n(v.grad) if v.grad is not None else zero(v)) for k, v in Pt.items()})
