"""Test-side restatements for the deep tower's dropout (include/dlamd.h "Dropout"), written
from the header's words, not from the kernels:

* philox4x32_10 / keep_mask: the mask in numpy;
* dnn_cate_fp64: `dnn_cate` (embedding -> tower -> head -> eps-log-loss) in float64 torch
  autograd with explicit masks, the reference the engine's gradients are compared against.
"""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
U32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """Philox-4x32-10 (Salmon et al., SC'11).  ctr: four uint32 arrays (x, y, z, w) of one
    shape, key: two uint32 scalars.  Returns the four output words, same shape."""
    c = [np.asarray(a, np.uint64) & U32 for a in ctr]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]
        p1 = np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & U32,
             (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & U32]
        k0 = (k0 + W0) & 0xFFFFFFFF
        k1 = (k1 + W1) & 0xFFFFFFFF
    return [a.astype(np.uint32) for a in c]


def keep_thr(keep):
    return min(int(np.floor(keep * 2.0 ** 32)), 2 ** 32 - 1)


def inv_keep(keep):
    """The scale the engine applies: float32(1) / float32(keep)."""
    return np.float32(1.0) / np.float32(keep)


def keep_mask(seed, step, layer, M, N, keep):
    """bool [M][N]: element (row, col) is kept iff word (col & 3) of
    Philox(counter (row, col >> 2, layer, step), key (seed low, seed high)) < keep_thr."""
    ng = (N + 3) // 4
    row = np.repeat(np.arange(M, dtype=np.uint64), ng).reshape(M, ng)
    cg = np.tile(np.arange(ng, dtype=np.uint64), M).reshape(M, ng)
    w = philox4x32_10([row, cg, np.full((M, ng), layer, np.uint64), np.full((M, ng), step, np.uint64)],
                      (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    words = np.stack(w, axis=2).reshape(M, 4 * ng)[:, :N]
    return words.astype(np.uint64) < np.uint64(keep_thr(keep))


def dnn_cate_fp64(cfg, P, batch, masks, invs):
    """dnn_cate in float64 autograd.  masks: len(hidden) + 1 bool arrays (tower input [B][S E],
    then each layer's output [B][h]); invs: their scales.  Returns logits z, the loss (with
    its L2 term), the gradients of every parameter (reference keys), and the engine's stage
    gradients: dh[l] = d loss / d (layer l's pre-activation), dx0 = d loss / d (the
    undropped tower input)."""
    import torch
    t = lambda a: torch.tensor(np.asarray(a, np.float64), dtype=torch.float64)
    S, E = cfg.S, cfg.E
    assert cfg.model == "dnn_cate" and cfg.V == 0
    Pt = {k: t(v).requires_grad_(True) for k, v in P.items()}
    lab = t(batch["label"]).reshape(-1)
    B = lab.shape[0]
    cate = torch.tensor(np.asarray(batch["cate_feats"], np.int64))[:, :S]
    V = torch.cat([torch.zeros(1, E, dtype=torch.float64), Pt["feats_emb"][1:]], 0)   # the zero row 0
    x0 = V[cate].reshape(B, S * E)
    x0.retain_grad()
    h = x0 * t(masks[0]) * float(invs[0])
    pres = []
    for i in range(len(cfg.hidden)):
        pre = h @ Pt["deep_%d" % i] + Pt["deep_bias_%d" % i]
        pre.retain_grad()
        pres.append(pre)
        h = torch.relu(pre) * t(masks[i + 1]) * float(invs[i + 1])
    z = (h @ Pt["deep_res"])[:, 0] + Pt["deep_res_bias"][0, 0]
    p = torch.sigmoid(z)
    eps = float(cfg.logloss_eps)
    per = -lab * torch.log(p + eps) - (1 - lab) * torch.log(1 - p + eps)
    loss = per.mean() + cfg.l2 * 0.5 * (Pt["deep_res"] ** 2).sum()
    loss.backward()
    n = lambda a: a.detach().numpy()
    return dict(z=n(z), loss=float(loss.detach()), G={k: n(v.grad) for k, v in Pt.items()},
                dh=[n(q.grad) for q in pres], dx0=n(x0.grad))
