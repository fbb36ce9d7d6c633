"""The side options of the dnn tower, one descriptor each, in the order of their launches.

Everything the package does per option is read from BRANCHES: ModelSpec's keywords, coercions and refusals,
local_run's key=value parsers and refusals, _ctr_model's hand-over, the two engines' "not supported by" lists,
CTREngine's parameter groups and their initialisers, and the logit chain's launches.  A descriptor is plain
data and a few small functions; each branch's limits (what its .hip file takes) stand once, beside its
`refusal`.  Numpy only: nothing here touches a device.
"""
import math
from functools import partial

import numpy as np

from .param_groups import (PNN_KEY, _shapes_pack, _shapes_unpack, afm_pack, afm_shapes, afm_unpack, autoint_shapes,
                           ccpm_shapes, cin_shapes, cross_pack, cross_unpack, pnn_pack, pnn_unpack)

# the models whose tower input the options join (all but batch_norm, which every f32 tower takes)
SIDE_MODELS = ("dnn_pipeline", "dnn_cate", "dnn_multi", "dnn_multi_cate")

CROSS_MAX_LAYERS, CROSS_MAX_IN = 4, 1024                                                  # csrc/cross.hip
AFM_MAX_ATT, AFM_MAX_FIELDS, AFM_EMB = 32, 64, (8, 16, 32)                                # csrc/afm.hip
CCPM_MAX_LAYERS, CCPM_MAX_FILTERS, CCPM_MAX_FIELDS, CCPM_EMB = 3, 8, 64, (8, 16, 32)      # csrc/ccpm.hip
CIN_MAX_LAYERS, CIN_MAX_MAPS, CIN_MAX_FIELDS, CIN_EMB, CIN_MAX_WEIGHTS = 3, 64, 64, (8, 16, 32), 262144   # csrc/cin.hip
AUTOINT_MAX_LAYERS, AUTOINT_HEADS, AUTOINT_DIMS, AUTOINT_MAX_FIELDS, AUTOINT_EMB = 3, (1, 2, 4), (8, 16, 32), 64, (8, 16, 32)   # csrc/autoint.hip
PNN_MAX_FIELDS, PNN_EMB = 64, (8, 16, 32)                                                 # csrc/pnn.hip
BI_MAX_FIELDS, BI_MAX_EMB = 64, 64                                                        # csrc/bi.hip (E a multiple of 4)


class Branch:
    """One side option.

    name         the ModelSpec keyword that switches it on (any true value), the word its refusals open with
    key          the engine's attribute, its ParamGroup's name and the stem of its entry points (dl_<key>_fwd)
    keywords     {ModelSpec keyword: default}, `name` first
    coerce       (*values) -> the values as ModelSpec stores them, or ValueError
    parse        (keyword, text) -> local_run's value, or SystemExit: the refusals that need the text alone
    refusal      (F, E, deep_in, *values) -> why the kernels do not take these values on F embedded fields of
                 size E and deep_in tower-input columns, without the option's name, or None
    phrases      _check_side_option's (joins, reads the f32 input, reads the undropped input); None: the option
                 is not one on the SIDE_MODELS' tower input
    sharded      ShardedCTREngine's reason
    shapes       (spec) -> {reference key: shape} in the device vector's order; or pack_pair: (spec) ->
                 (n, pack, unpack).  Neither: no ParamGroup
    ckpt_keys    the Adam moments' names in a checkpoint
    reg          (spec) -> the count of leading values under the loss's L2 term; None: no regulariser
    init         (rng, spec, unpack) -> reference-layout initial values
    lead         (spec) -> the launches' own leading arguments (the engine keeps them alive): a member of the
                 logit chain
    state        (spec, B) -> the shape of the forward's private state the backward reads, or absent
    whole_x0     the branch reads every tower-input column: no x0 column and no z_in argument, dx0's window given
    """

    def __init__(self, name, key, keywords, coerce, parse, sharded, refusal=None, phrases=None, shapes=None,
                 pack_pair=None, ckpt_keys=None, reg=None, init=None, lead=None, state=None, whole_x0=False):
        self.__dict__.update({k: v for k, v in locals().items() if k != "self"})

    def values(self, holder):
        """The keywords' values on a ModelSpec or a local_run ModelParams (defaults where absent)."""
        return [getattr(holder, k, d) for k, d in self.keywords.items()]

    def layout(self, sp):
        """(n, pack, unpack) of the option's parameter vector."""
        if self.pack_pair:
            return self.pack_pair(sp)
        shapes = self.shapes(sp)
        return (sum(int(np.prod(shp)) for shp in shapes.values()),
                partial(_shapes_pack, shapes=shapes, what=self.name + ": "), partial(_shapes_unpack, shapes=shapes))


def _slashes(values):
    return " / ".join(map(str, values))


# ---------------------------------------------------------------------------------- coercions (ModelSpec)
def _count(name):
    def coerce(v):
        if int(v) != v or v < 0:
            raise ValueError("%s must be an integer >= 0, got %r" % (name, v))
        return (int(v),)
    return coerce


def _int_seq(name):
    def coerce(v):
        try:
            seq = tuple(v)
            ok = all(int(c) == c for c in seq)
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise ValueError("%s must be a sequence of integers, got %r" % (name, v))
        return (tuple(int(c) for c in seq),)
    return coerce


def _autoint_coerce(*values):
    for k, v in zip(("autoint_layers", "autoint_heads", "autoint_dim"), values):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError("autoint_layers: %s must be an integer, got %r" % (k, v))
    return tuple(int(v) for v in values)


def _pnn_coerce(v):
    if v == "outer":
        raise ValueError("pnn='outer': the outer-product layer (PNN.py:85-91, an E * E first-layer input) is "
                         "not built; pnn='inner' is")
    if v not in (None, "inner"):
        raise ValueError("pnn must be None or 'inner', got %r" % (v,))
    return (v,)


def _bn_coerce(on, eps, momentum):
    e, m = float(eps), float(momentum)
    if not (math.isfinite(e) and e > 0.0):
        raise ValueError("batch_norm: bn_eps must be finite and > 0, got %r" % (eps,))
    if not 0.0 < m <= 1.0:
        raise ValueError("batch_norm: bn_momentum must lie in (0, 1], got %r" % (momentum,))
    return bool(on), e, m


# ---------------------------------------------------------------------------------- parsers (local_run)
def _parse_count(name, hi):
    def parse(k, v):
        try:
            n = int(v)
        except ValueError:
            raise SystemExit("%s=%s is not an integer" % (name, v))
        if not 0 <= n <= hi:
            raise SystemExit("%s=%s must lie in [0, %d]" % (name, v, hi))
        return n
    return parse


def _parse_seq(name, max_len, hi):
    def parse(k, v):
        try:
            f = [int(x) for x in v.split(",")]
        except ValueError:
            raise SystemExit("%s=%s is not a comma-separated list of integers" % (name, v))
        if not 1 <= len(f) <= max_len or not all(1 <= c <= hi for c in f):
            raise SystemExit("%s=%s must hold 1 to %d values in [1, %d]" % (name, v, max_len, hi))
        return f
    return parse


def _parse_flag(k, v):
    if v not in ("0", "1"):
        raise SystemExit("%s=%s must be 0 or 1" % (k, v))
    return v == "1"


def _autoint_parse(k, v):
    try:       # the accepted shapes depend on all three and on the fields: the refusal, once those are counted
        return int(v)
    except ValueError:
        raise SystemExit("autoint_layers: %s=%s is not an integer" % (k, v))


def _pnn_parse(k, v):
    if v == "outer":
        raise SystemExit("pnn=outer: the outer-product layer is not built; pnn=inner is")
    if v != "inner":
        raise SystemExit("pnn=%s must be inner" % v)
    return v


def _bn_parse(k, v):
    if k == "batch_norm":
        return _parse_flag(k, v)
    try:
        x = float(v)
    except ValueError:
        raise SystemExit("%s=%s is not a number" % (k, v))
    if not (0.0 < x < float("inf")) or (k == "bn_momentum" and x > 1.0):
        raise SystemExit("%s=%s must %s" % (k, v, "lie in (0, 1]" if k == "bn_momentum" else "be finite and > 0"))
    return x


# ---------------------------------------------------------------------------------- refusals (both)
def _cross_refusal(F, E, deep_in, L):
    if L > CROSS_MAX_LAYERS or deep_in > CROSS_MAX_IN:
        return ("at most %d layers on at most %d tower-input columns, got %d on %d"
                % (CROSS_MAX_LAYERS, CROSS_MAX_IN, L, deep_in))


def _afm_refusal(F, E, deep_in, A):
    if A > AFM_MAX_ATT or not 2 <= F <= AFM_MAX_FIELDS or E not in AFM_EMB:
        return ("at most %d attention units on 2 to %d embedded fields of size %s, got %d on %d fields of size %d"
                % (AFM_MAX_ATT, AFM_MAX_FIELDS, _slashes(AFM_EMB), A, F, E))


def _ccpm_refusal(F, E, deep_in, filters):
    Lc = len(filters)
    if (Lc > CCPM_MAX_LAYERS or not all(1 <= c <= CCPM_MAX_FILTERS for c in filters)
            or not 2 <= F <= CCPM_MAX_FIELDS or E not in CCPM_EMB or (F >> Lc) < 1 or (E >> Lc) < 1):
        return ("1 to %d layers of 1 to %d filters on 2 to %d embedded fields of size %s, every layer halving the "
                "map to at least 1 x 1; got %r on %d fields of size %d"
                % (CCPM_MAX_LAYERS, CCPM_MAX_FILTERS, CCPM_MAX_FIELDS, _slashes(CCPM_EMB), tuple(filters), F, E))


def cin_weights(F, layers):
    """The CIN's layer weights: sum_k H_k H_{k-1} F, H_0 = F."""
    H = (F,) + tuple(layers)
    return sum(H[k + 1] * H[k] * F for k in range(len(layers)))


def _cin_refusal(F, E, deep_in, layers):
    nw = cin_weights(F, layers)
    if (len(layers) > CIN_MAX_LAYERS or not all(1 <= h <= CIN_MAX_MAPS for h in layers)
            or not 2 <= F <= CIN_MAX_FIELDS or E not in CIN_EMB or nw > CIN_MAX_WEIGHTS):
        return ("1 to %d layers of 1 to %d feature maps on 2 to %d embedded fields of size %s, at most %d layer "
                "weights; got %r on %d fields of size %d (%d weights)"
                % (CIN_MAX_LAYERS, CIN_MAX_MAPS, CIN_MAX_FIELDS, _slashes(CIN_EMB), CIN_MAX_WEIGHTS, tuple(layers),
                   F, E, nw))


def _autoint_refusal(F, E, deep_in, L, Hn, D):
    if not (1 <= L <= AUTOINT_MAX_LAYERS and Hn in AUTOINT_HEADS and D in AUTOINT_DIMS and D // Hn >= 2
            and 2 <= F <= AUTOINT_MAX_FIELDS and E in AUTOINT_EMB):
        return ("1 to %d layers of autoint_heads in %s on autoint_dim in %s columns with at least 2 a head, on 2 to "
                "%d embedded fields of size %s; got autoint_layers=%d autoint_heads=%d autoint_dim=%d on %d fields "
                "of size %d" % (AUTOINT_MAX_LAYERS, _slashes(AUTOINT_HEADS), _slashes(AUTOINT_DIMS),
                                AUTOINT_MAX_FIELDS, _slashes(AUTOINT_EMB), L, Hn, D, F, E))


def _pnn_refusal(F, E, deep_in, v):
    if not 2 <= F <= PNN_MAX_FIELDS or E not in PNN_EMB:
        return "2 to %d embedded fields of size %s, got %d fields of size %d" % (PNN_MAX_FIELDS, _slashes(PNN_EMB), F, E)


def _bi_refusal(F, E, deep_in, on):
    if not 2 <= F <= BI_MAX_FIELDS or E % 4 or not 4 <= E <= BI_MAX_EMB:
        return ("2 to %d embedded fields of a size that is a multiple of 4 in [4, %d], got %d fields of size %d"
                % (BI_MAX_FIELDS, BI_MAX_EMB, F, E))


# ---------------------------------------------------------------------------------- layouts and initialisers
def _cross_pair(sp):
    lay = dict(L=sp.cross_layers, D0=sp.deep_in, rows=sp.x0_ref_rows())
    return (2 * sp.cross_layers + 1) * sp.deep_in, partial(cross_pack, **lay), partial(cross_unpack, **lay)


def _pnn_pair(sp):
    lay = dict(D1=sp.hidden[0], F=sp.afm_fields)
    return lay["D1"] * lay["F"], partial(pnn_pack, **lay), partial(pnn_unpack, **lay)


def _afm_pair(sp):
    lay = dict(E=sp.E, A=sp.afm_attention)
    return sum(int(np.prod(shp)) for shp in afm_shapes(**lay).values()), partial(afm_pack, **lay), partial(afm_unpack, **lay)


def _ccpm_shapes(sp):
    return ccpm_shapes(sp.ccpm_dims())


def _cin_shapes(sp):
    return cin_shapes(sp.afm_fields, sp.cin_layers)


def _autoint_shapes(sp):
    return autoint_shapes(sp.afm_fields, sp.E, sp.autoint_layers, sp.autoint_dim)


def _cross_init(rng, sp, unpack):
    """DCN.py:75-79 cross_layer / cross_bias ~ N(0, sqrt(2 / (D + D))); :90-93 the output layer's cross part
    ~ N(0, sqrt(2 / (D + H + 1))).  Drawn in the device vector's own column order."""
    D, Lc = sp.deep_in, sp.cross_layers
    v = rng.standard_normal((2 * Lc + 1, D)) * math.sqrt(2.0 / (D + D))
    v[0] = rng.standard_normal(D) * math.sqrt(2.0 / (D + sp.hidden[-1] + 1))
    return unpack(v.astype(np.float32).reshape(-1))


def _afm_init(rng, sp, unpack):
    """AFM.py:75-85: attention_w, attention_b ~ N(0, sqrt(2 / (A + E))); attention_h, attention_p ~ N(0, 1)."""
    A, g = sp.afm_attention, math.sqrt(2.0 / (sp.afm_attention + sp.E))
    return {"attention_w": rng.standard_normal((sp.E, A)) * g, "attention_b": rng.standard_normal((1, A)) * g,
            "attention_h": rng.standard_normal((1, A)), "attention_p": rng.standard_normal((sp.E, 1))}


def _ccpm_init(rng, sp, unpack):
    """Keras' defaults (CCPM.py:56-68 passes no initializer): glorot_uniform kernels, zero biases."""
    P = {}
    for k, shp in _ccpm_shapes(sp).items():
        if k.endswith(".bias"):
            P[k] = np.zeros(shp, np.float32)
        else:
            rf = shp[0] * shp[1] if len(shp) == 4 else 1
            lim = math.sqrt(6.0 / (rf * (shp[-2] + shp[-1])))
            P[k] = rng.uniform(-lim, lim, shp)
    return P


def _glorot_res_init(shapes):
    """Matrices glorot-uniform (fan-in rows, fan-out columns); the output layer's part <x>_res [n, 1] ~
    N(0, sqrt(2 / (n + 1))) as deep_res: the CIN and AutoInt."""
    def init(rng, sp, unpack):
        P = {}
        for k, shp in shapes(sp).items():
            if k.endswith("_res"):
                P[k] = rng.standard_normal(shp) * math.sqrt(2.0 / (shp[0] + 1))
            else:
                lim = math.sqrt(6.0 / (shp[0] + shp[1]))
                P[k] = rng.uniform(-lim, lim, shp)
        return P
    return init


def _pnn_init(rng, sp, unpack):
    """PNN.py:57: product-quadratic-inner ~ N(0, 0.01)."""
    return {PNN_KEY: rng.standard_normal((sp.hidden[0], sp.afm_fields)) * 0.01}


def _int3(values):
    import ctypes
    return (ctypes.c_int32 * 3)(*values)


_FLAT = "gradients are not part of the flat all-reduce"
_BRANCH_READS = ("the branch reads the f32 tower input", "the branch reads the undropped fields")

BRANCHES = (
    # Deep & Cross network (csrc/cross.hip): [c | w_0 .. | b_0 ..] in x0's column order, the forward's s [B, L];
    # L2 on c, the output layer's cross part (DCN.py:104)
    Branch("cross_layers", "cross", {"cross_layers": 0}, _count("cross_layers"),
           _parse_count("cross_layers", CROSS_MAX_LAYERS), "the cross parameters' " + _FLAT, _cross_refusal,
           ("the cross network joins", "the cross network reads the f32 tower input",
            "the cross network reads the undropped input"),
           pack_pair=_cross_pair, ckpt_keys=("adam/cm", "adam/cv"), reg=lambda sp: sp.deep_in, init=_cross_init,
           lead=lambda sp: (sp.deep_in, sp.cross_layers), state=lambda sp, B: (B, sp.cross_layers),
           whole_x0=True),
    # attentional interactions (csrc/afm.hip): [p (E) | h (A) | b (A) | W (E A)], the forward's softmax
    # statistics [B, 2]; no regulariser (AFM.py:137 has none on these variables)
    Branch("afm_attention", "afm", {"afm_attention": 0}, _count("afm_attention"),
           _parse_count("afm_attention", AFM_MAX_ATT), "the attention parameters' " + _FLAT, _afm_refusal,
           ("the attentional interactions join",) + _BRANCH_READS,
           pack_pair=_afm_pair, ckpt_keys=("adam/am", "adam/av"), init=_afm_init,
           lead=lambda sp: (sp.afm_fields, sp.E, sp.afm_attention), state=lambda sp, B: (B, 2)),
    # CCPM branch (csrc/ccpm.hip): [p | K_0 | b_0 | K_1 | b_1 ..]; no regulariser (CCPM.py:73-74)
    Branch("ccpm_filters", "ccpm", {"ccpm_filters": ()}, _int_seq("ccpm_filters"),
           _parse_seq("ccpm_filters", CCPM_MAX_LAYERS, CCPM_MAX_FILTERS), "the convolution parameters' " + _FLAT,
           _ccpm_refusal, ("the convolutional interactions join",) + _BRANCH_READS,
           shapes=_ccpm_shapes, ckpt_keys=("adam/km", "adam/kv"), init=_ccpm_init,
           lead=lambda sp: (sp.afm_fields, sp.E, len(sp.ccpm_filters), _int3(sp.ccpm_filters))),
    # compressed interaction network (csrc/cin.hip): [c | W^1 | W^2 ..]; L2 on c = cin_res as on cross_res
    Branch("cin_layers", "cin", {"cin_layers": ()}, _int_seq("cin_layers"),
           _parse_seq("cin_layers", CIN_MAX_LAYERS, CIN_MAX_MAPS), "the interaction network's parameters' " + _FLAT,
           _cin_refusal, ("the compressed interaction network joins",) + _BRANCH_READS,
           shapes=_cin_shapes, ckpt_keys=("adam/nm", "adam/nv"), reg=lambda sp: sum(sp.cin_layers),
           init=_glorot_res_init(_cin_shapes),
           lead=lambda sp: (sp.afm_fields, sp.E, len(sp.cin_layers), _int3(sp.cin_layers))),
    # AutoInt's interacting layers (csrc/autoint.hip): [w | Wq_1 | Wk_1 | Wv_1 | Wr_1 | Wq_2 ..]; the backward
    # recomputes in LDS and keeps nothing in HBM; L2 on w = autoint_res as on cin_res.  0 layers: off, whatever
    # the other two keywords say
    Branch("autoint_layers", "autoint", {"autoint_layers": 0, "autoint_heads": 2, "autoint_dim": 16},
           _autoint_coerce, _autoint_parse, "the interacting layers' parameters' " + _FLAT, _autoint_refusal,
           ("the interacting layers join",) + _BRANCH_READS,
           shapes=_autoint_shapes, ckpt_keys=("adam/im", "adam/iv"), reg=lambda sp: sp.afm_fields * sp.autoint_dim,
           init=_glorot_res_init(_autoint_shapes),
           lead=lambda sp: (sp.afm_fields, sp.E, sp.autoint_layers, sp.autoint_heads, sp.autoint_dim)),
    # product layer (csrc/pnn.hip): theta [D1, F], launched inside the tower; no regulariser (PNN.py:136-139)
    Branch("pnn", "pnn", {"pnn": None}, _pnn_coerce, _pnn_parse, "theta's gradient is not part of the flat all-reduce",
           _pnn_refusal, ("the product layer feeds", "the product layer reads the f32 tower input and finishes the "
                          "f32 first layer", "the product layer reads the undropped fields"),
           pack_pair=_pnn_pair, ckpt_keys=("adam/pm", "adam/pv"), init=_pnn_init),
    # Bi-Interaction pooling (csrc/bi.hip): E more tower-input columns, no parameter
    Branch("bi_interaction", "bi", {"bi_interaction": False}, lambda v: (bool(v),), _parse_flag,
           "its step does not launch the pooling's kernels around the first tower layer", _bi_refusal,
           ("the Bi-Interaction pooling feeds", "the pooling reads and extends the f32 tower input",
            "the pooling's backward reads the undropped fields")),
    # batch normalisation (csrc/bn.hip): every model with an f32 tower; its per-layer groups are the engine's
    Branch("batch_norm", "bn", {"batch_norm": False, "bn_eps": 1e-5, "bn_momentum": 0.1}, _bn_coerce, _bn_parse,
           "the batch statistics would need a reduction across the ranks"),
)

KEYWORDS = {k: b for b in BRANCHES for k in b.keywords}      # every side keyword -> its option


def unsupported(spec, cls):
    """Refuses (ValueError) the first option that is on, for the engine classes whose step carries none of them."""
    for b in BRANCHES:
        if getattr(spec, b.name):
            raise ValueError("%s: not supported by %s (%s)" % (b.name, cls, b.sharded))
