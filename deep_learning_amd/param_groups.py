"""The small dense parameter vectors beside the deep tower (cross network, attentional interactions,
CCPM branch, compressed interaction network, AutoInt's interacting layers, product layer, batch norm's [gamma | beta]): their host layouts and their device life cycle.

Every one of them is a flat f32 vector padded to 4 with two Adam moment vectors, a slab of per-block
partial gradient sums [dl_<x>_grid(max_batch), n] its backward kernel fills, and one dl_adam_dense
launch per step.  The layouts are pure host functions (numpy in, numpy out) between the reference's keys
and shapes and the device vector; ParamGroup holds the buffers and does the rest.
"""
from functools import partial

import numpy as np
import torch

from . import _lib
from ._lib import ptr


def _ru(x, m):
    return (x + m - 1) // m * m


def _shapes_pack(P, shapes, what=""):
    """Reference-layout parameters P and {key: shape} in the device vector's order -> the concatenated
    vector; a variable of another size is refused, the message opening with `what` (the option's name)."""
    parts = []
    for k, shp in shapes.items():
        a = np.asarray(P[k], np.float32)
        if a.size != int(np.prod(shp)):
            raise ValueError("%s%s holds %d values, not %s" % (what, k, a.size, " x ".join(map(str, shp))))
        parts.append(a.reshape(-1))
    return np.concatenate(parts)


def _shapes_unpack(v, shapes):
    """Inverse of _shapes_pack: {key: numpy in the reference's shape}."""
    out, o = {}, 0
    for k, shp in shapes.items():
        n = int(np.prod(shp))
        out[k] = np.asarray(v[o:o + n], np.float32).reshape(shp).copy()
        o += n
    return out


def cross_keys(L):
    """Reference keys of the cross vector's (2L + 1) parts, in its order [c | w_l | b_l]."""
    return ("cross_res",) + tuple("cross_layer_%d" % l for l in range(L)) + tuple("cross_bias_%d" % l for l in range(L))


def cross_pack(P, L, D0, rows):
    """Reference-layout cross parameters ([D, 1] each, rows in the reference's deep-input order) -> the
    device vector (x0's column order; rows = ModelSpec.x0_ref_rows())."""
    parts = []
    for k in cross_keys(L):
        a = np.asarray(P[k], np.float32).reshape(-1)
        if a.size != D0:
            raise ValueError("%s holds %d values for %d tower-input columns" % (k, a.size, D0))
        parts.append(a[rows])
    return np.concatenate(parts)


def cross_unpack(v, L, D0, rows):
    """Inverse of cross_pack: {key: [D, 1] numpy}."""
    v = np.asarray(v, np.float32).reshape(2 * L + 1, D0)
    out = {}
    for i, k in enumerate(cross_keys(L)):
        a = np.empty(D0, np.float32)
        a[rows] = v[i]
        out[k] = a[:, None]
    return out


def afm_shapes(E, A):
    """The attention variables (AFM.py:75-85) in the device vector's order [p | h | b | W]."""
    return {"attention_p": (E, 1), "attention_h": (1, A), "attention_b": (1, A), "attention_w": (E, A)}


def ccpm_shapes(dims):
    """ModelSpec.ccpm_dims() -> {variable: Keras shape} in the device vector's order: ccpm_out.kernel
    [H_L W_L C_L, 1], then per layer ccpm_conv_{l}.kernel [3, 3, C_{l-1}, C_l] and ccpm_conv_{l}.bias [C_l]."""
    out = {"ccpm_out.kernel": (dims[-1][0] * dims[-1][1] * dims[-1][2], 1)}
    for l in range(len(dims) - 1):
        out["ccpm_conv_%d.kernel" % l] = (3, 3, dims[l][2], dims[l + 1][2])
        out["ccpm_conv_%d.bias" % l] = (dims[l + 1][2],)
    return out


def cin_shapes(F, layers):
    """The CIN variables in the device vector's order [c | W^1 | W^2 ..]: cin_res [sum H_k, 1], then per
    layer cin_layer_{k-1} [H_{k-1} F, H_k] (row i F + j; H_0 = F)."""
    out = {"cin_res": (sum(layers), 1)}
    H = (F,) + tuple(layers)
    for k in range(len(layers)):
        out["cin_layer_%d" % k] = (H[k] * F, H[k + 1])
    return out


def autoint_shapes(F, E, L, D):
    """The AutoInt variables in the device vector's order [w | Wq_1 | Wk_1 | Wv_1 | Wr_1 | Wq_2 ..]:
    autoint_res [F D, 1], then per layer autoint_q_{l-1}, autoint_k_{l-1}, autoint_v_{l-1}, autoint_r_{l-1}
    [D_{l-1}, D] (D_0 = E, D_l = D)."""
    out = {"autoint_res": (F * D, 1)}
    for l in range(L):
        for m in "qkvr":
            out["autoint_%s_%d" % (m, l)] = (D if l else E, D)
    return out


# the pack / unpack names of the shapes layouts, for callers outside the package: _shapes_pack with the
# option's name as the refusal's prefix, and its inverse
ccpm_pack, cin_pack, autoint_pack = (partial(_shapes_pack, what=w + ": ")
                                     for w in ("ccpm_filters", "cin_layers", "autoint_layers"))
ccpm_unpack = cin_unpack = autoint_unpack = _shapes_unpack


def afm_pack(P, E, A):
    return _shapes_pack(P, afm_shapes(E, A))


def afm_unpack(v, E, A):
    return _shapes_unpack(v, afm_shapes(E, A))


PNN_KEY = "product-quadratic-inner"   # PNN.py:57, [D1, F]: the device vector is its row-major image


def pnn_pack(P, D1, F):
    """Reference-layout theta [D1, F] -> the device vector."""
    a = np.asarray(P[PNN_KEY], np.float32)
    if a.shape != (D1, F):
        raise ValueError("%s has shape %r, not (%d, %d)" % (PNN_KEY, a.shape, D1, F))
    return np.ascontiguousarray(a).reshape(-1)


def pnn_unpack(v, D1, F):
    """Inverse of pnn_pack."""
    return {PNN_KEY: np.asarray(v, np.float32).reshape(D1, F).copy()}


BN_KEY = "batch_norm_%d.%s"   # NFM.py:166: setattr(self, 'batch_norm_' + str(i), ...), i from 1


def bn_vec(P, l, part, D, default=None):
    """Hidden layer l's batch-norm vector `part` [D] of P (absent, with a default: filled with it)."""
    k = BN_KEY % (l + 1, part)
    if k not in P and default is not None:
        return np.full(D, default, np.float32)
    a = np.ascontiguousarray(P[k], np.float32).reshape(-1)
    if a.size != D:
        raise ValueError("%s holds %d values for %d units" % (k, a.size, D))
    return a


def bn_pack(P, l, D):
    """Reference-layout gamma and beta of hidden layer l -> the device vector [gamma | beta]."""
    return np.concatenate([bn_vec(P, l, "weight", D), bn_vec(P, l, "bias", D)])


def bn_unpack(v, l, D):
    """Inverse of bn_pack."""
    v = np.asarray(v, np.float32)
    return {BN_KEY % (l + 1, "weight"): v[:D].copy(), BN_KEY % (l + 1, "bias"): v[D:].copy()}


class ParamGroup:
    """One flat dense parameter vector on the device: w with its Adam moments m and v (zeros, n padded
    to 4) and the slab [blocks, n] of per-block partial gradient sums, blocks = grid_fn(max_batch) rows of
    capacity (a step of B samples fills and sums grid_fn(B) of them).

    pack(P) -> np.float32[n] and unpack(vec[n]) -> {key: array} convert between the reference's keys and
    layout and the vector; ckpt_keys name the moments in a checkpoint file; reg = (l2, l2n, reg_sum) are
    dl_adam_dense's regulariser arguments (L2 on the first l2n values, its sum of squares added to the
    reg_sum tensor)."""

    def __init__(self, name, n, grid_fn, max_batch, device, pack, unpack, ckpt_keys, reg=(0.0, 0, None)):
        self.name, self.n, self.grid_fn = name, n, grid_fn
        self.pack, self.unpack, self.ckpt_keys, self.reg = pack, unpack, ckpt_keys, reg
        self.w, self.m, self.v = (torch.zeros(_ru(n, 4), dtype=torch.float32, device=device) for _ in range(3))
        self.blocks = self.rows(max_batch)
        self.slab = torch.zeros(self.blocks, n, dtype=torch.float32, device=device)

    def rows(self, B):
        """Slab rows a backward over B samples writes."""
        return getattr(_lib.lib(), self.grid_fn)(B)

    def load(self, P):
        """Reference-layout parameters -> w."""
        self.w[: self.n].copy_(torch.from_numpy(self.pack(P)))

    def export(self, which):
        """w, m or v in the reference's keys and shapes."""
        return self.unpack(getattr(self, which)[: self.n].cpu().numpy())

    def adam(self, engine, B, s):
        """The step's Adam update from the slab rows the backward over B samples wrote."""
        l2, l2n, reg_sum = self.reg
        engine._c("adam_" + self.name, "dl_adam_dense", ptr(self.w), ptr(self.m), ptr(self.v), ptr(self.slab),
                  self.rows(B), self.n, self.n, l2, l2n, ptr(engine.opt), None, ptr(reg_sum), s)
