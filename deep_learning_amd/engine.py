"""MI355X training engine for the reference's CTR models (DeepFM / DNN / Wide&Deep).

One ``CTREngine`` holds every device buffer of a model (parameters, TF1-Adam
state, activations, gradient tables, partial-sum slabs) and runs a training
step as a fixed sequence of HIP kernels from ``libdlamd.so`` on one stream —
so the whole step can be captured into a hipGraph and replayed.

Step (deepfm_pipeline, reference models/deepfm_pipeline.py:76-191):
  adam_begin_step                       alpha_t, beta powers, global_step
  embed_fwd                             gather + FM 1st/2nd order + x0 assembly
  gemm_f32 x L (ReLU)                   deep tower forward (bias = ones column)
  head_fwd_bwd                          logit, sigmoid, log-loss, dz, dh_L, dW_head partials
  for l = L-1..0: gemm dW (split-K) ; gemm dX (ReluGrad) ; adam_dense(W_l)
  embed_bwd + cont_reduce               FM/deep row gradients -> dense gradient table
  adam_dense(head) ; adam_rows(table) ; adam_rows(first-order)

Internal layouts (import/export map to the reference's):
  x0  = [cate embeddings (S*E) | pooled (M*E) | cont (C) | vector (V) | 1 | 0-pad]
  W_l = [in_ld, out_ld] row-major; row in_dim holds the bias, pads are zero
  head w = [first (F) | second (E) | deep (H) | bias]   (deepfm; dnn: [H | bias])
"""
import contextlib
import gc
import math
import os
import time
from functools import partial
from types import SimpleNamespace

import numpy as np
import torch

from . import _lib, branches
from ._lib import call, ptr
from .branches import BRANCHES, SIDE_MODELS
from .param_groups import BN_KEY, ParamGroup, _ru, bn_pack, bn_unpack, bn_vec
from .param_groups import ccpm_pack, ccpm_shapes, ccpm_unpack  # noqa: F401  (read from here outside the package)

F32 = torch.float32


# Model families of the reference's pipeline-style model files:
#   fm     FM first/second order feeds the head (deepfm_*), else the deep_res head (dnn_*)
#   cont   dense features present; "first": FM cont rows 0..C-1, cate ids at +C
#          (deepfm_pipeline.py:58-61,89); "last": FM cont rows at cate_index_size + j,
#          ids unshifted (deepfm_multi.py:139); "deep": cont only in the deep input (dnn_*)
#   multi  nonzero-mean-pooled multi-hot slots after the S singles
FAMILIES = {
    "deepfm_pipeline": dict(fm=True, cont="first", multi=False),     # models/deepfm_pipeline.py:76-191
    "deepfm_cate": dict(fm=True, cont=None, multi=False),            # models/deepfm_cate.py:73-169
    "deepfm_multi_cate": dict(fm=True, cont=None, multi=True),       # models/deepfm_multi_cate.py:113-240
    "deepfm_multi": dict(fm=True, cont="last", multi=True),          # models/deepfm_multi.py:124-260
    "dnn_pipeline": dict(fm=False, cont="deep", multi=False),        # models/dnn_pipeline.py:68-137
    "dnn_cate": dict(fm=False, cont=None, multi=False),              # models/dnn_cate.py:62-131
    "dnn_multi": dict(fm=False, cont="deep", multi=True),            # models/dnn_multi.py:70-167
    "dnn_multi_cate": dict(fm=False, cont=None, multi=True),         # models/dnn_multi_cate.py:64-162
    "wdl": dict(fm=False, cont="deep", multi=False),                 # models/wdl.py:123-285
    # load-style models (int32 ids, no zero row):
    #   deepfm: FM fields [cate | cont] with cont rows at cate_field_size + j (deepfm.py:66-73)
    #   dnn:    xavier 'weight_mat' table, L1 on every hidden weight (dnn.py:49-52,88-90)
    "deepfm": dict(fm=True, cont="field", multi=False),              # models/deepfm.py:39-162
    "dnn": dict(fm=False, cont="deep", multi=False),                 # models/dnn.py:35-96
}


class ModelSpec:
    """Shape/hyper-parameter description of one reference model.

    model: a key of FAMILIES (the reference's pipeline-style model files + wdl)
    C cont fields, V vector size, S single cate fields, E embedding size,
    cate_index_size (reference `cate_feats_size`), hidden units, multi_ranges
    [[start, end, name], ...] (multi-hot slots, relative to the multi block), Fw wide
    ids (wdl), lr, l2, decay_steps/decay_rate (exponential_decay), Adam betas/eps.
    dropout_keep_deep: the reference's keep probabilities of the deep tower (tf.nn.dropout after
    the tower input and after every ReLU layer, deepfm_pipeline.py:148-153): len(hidden) + 1
    values in (0, 1], a longer list truncated (the reference's default holds 5 entries for 3
    layers); None or all ones: no dropout.
    dropout_keep_fm: the reference's keep probabilities of the FM part (tf.nn.dropout on the
    first-order products and on the second-order vector, deepfm_pipeline.py:98,110): two values in
    (0, 1], a longer list truncated; None, with no effect, for all ones and for the models without
    an FM part (dnn*, wdl), whose reference classes never read it.
    pos_weight: the loss weight of a positive sample relative to a negative one (finite, > 0;
    tf.losses.log_loss's weights= with w_b = weight_b * (1 + (pos_weight - 1) * y_b), which the
    reference leaves at 1); anything but 1 turns the engine's sample weighting on
    (CTREngine(sample_weight=...)).
    cross_layers: layers of a Deep & Cross network (test_model/DCN.py:73-96) on the tower input of
    the dnn_pipeline / dnn_cate / dnn_multi / dnn_multi_cate models, its output joining the tower's
    in the one output layer (parameters cross_layer_%d, cross_bias_%d, cross_res); 0: none.
    afm_attention: attention units A of an attentional pairwise-interaction branch (the
    Pair-wise_Interaction_Layer and attention_net of test_model/AFM.py:63-129) over the S + M
    embedded fields of the same four models, its logit added to the tower's (and the cross
    network's); parameters attention_w [E, A], attention_b [1, A], attention_h [1, A],
    attention_p [E, 1], no regulariser; 0: none.
    pnn: "inner" puts the inner-product layer of test_model/PNN.py:78-83 in front of the same four
    models' tower: lp_i = || sum_f theta[i, f] e_f || over the S + M embedded fields, added to layer
    0's pre-activation before its ReLU (hidden[0] = D1); parameter product-quadratic-inner [D1, F],
    no regulariser; the reference's product-linear and product-bias are layer 0 itself; None: off
    (DESIGN 4m).
    batch_norm: batch normalisation (test_model/NFM.py:160-167, 244-252: nn.BatchNorm1d, torch's
    defaults bn_eps = 1e-5, bn_momentum = 0.1) between every hidden layer's linear part and its ReLU,
    for every model with an f32 tower: training steps normalise by the batch's unweighted statistics
    and update the running ones, predict uses the running ones; per hidden layer l the parameters
    batch_norm_{l+1}.weight / .bias [D] (Adam, no regulariser) and the state batch_norm_{l+1}.running_mean
    / .running_var [D]; False: none.
    bi_interaction: True adds the Bi-Interaction pooling of test_model/NFM.py:192-197, 226 to the same four
    models' tower input: q = sum_{f<g} e_f * e_g over the S + M embedded fields, E more columns after the
    reference's [cont, vector, single cate, pooled] (deep_0 becomes [deep_in, hidden[0]] with deep_in
    grown by E); no new parameter; with batch_norm=True the reference's NFM; False: none.
    ccpm_filters: the channels (C_0, .., C_{L-1}) of a CCPM branch (test_model/CCPM.py:45-68) beside the same
    four models' tower: L times Conv2D(3x3, same, relu) + MaxPool2D(2x2) on the [E, F] map of the S + M
    embedded fields, Flatten, Dense(1) without its bias, its logit added to the tower's (after the cross
    network's and the attentional interactions'); parameters ccpm_conv_{l}.kernel [3, 3, C_{l-1}, C_l],
    ccpm_conv_{l}.bias [C_l], ccpm_out.kernel [H_L W_L C_L, 1], no regulariser; (): none.
    cin_layers: the feature maps (H_1, .., H_L) of a Compressed Interaction Network (xDeepFM, Lian et al. 2018,
    eq. 6-8: direct form, identity activation, no bias, no split-half) beside the same four models' tower:
    X^k[h] = sum_{i, j} W^k[h, i, j] X^{k-1}[i] * X^0[j] over the S + M embedded fields X^0, every map
    sum-pooled over the embedding and projected by cin_res, its logit added to the tower's (after the cross
    network's, the attentional interactions' and the CCPM branch's); parameters cin_layer_{k-1}
    [H_{k-1} F, H_k] (row i F + j, H_0 = F) and cin_res [sum H_k, 1], the loss's L2 term on cin_res as on
    cross_res; (): none.
    autoint_layers, autoint_heads, autoint_dim: L stacked interacting layers of AutoInt (Song et al. 2019, eq.
    5-8) beside the same four models' tower, Hn heads on D columns (d = D / Hn a head): with X^0 the S + M
    embedded fields [F, E], X^l = relu(concat_h softmax(Q_h K_h^T) V_h + X^{l-1} Wr_l), Q, K, V = X^{l-1} Wq_l,
    Wk_l, Wv_l (unscaled scores, no bias), X^L projected by autoint_res, its logit added to the tower's last
    (after every other branch's); parameters autoint_{q,k,v,r}_{l-1} [D_{l-1}, D] (D_0 = E) and autoint_res
    [F D, 1], the loss's L2 term on autoint_res as on cin_res; L in 1..3, Hn in 1 / 2 / 4, D in 8 / 16 / 32 with
    D / Hn >= 2; autoint_layers=0 (the default, with heads 2 and dim 16): none.
    wide_optimizer: "adam" (the reference's one optimizer) or "ftrl" (wdl only): wdl_weights trained
    by TF1 FtrlOptimizer(wide_lr, learning_rate_power=-0.5, initial_accumulator_value=0.1,
    l1_regularization_strength=wide_l1, l2_regularization_strength=wide_l2), the loss's L2 term on
    wdl_weights dropped; wide_lr None: lr, and never decayed.
    """

    MAX_SLOTS, MAX_FM_CONT, REC_FWD_MAX_FM = 128, 32, 64     # csrc/embed.hip: kMaxSlots, kMaxHotCont, dl_embed_fwd_rec_flat
    MAX_FM_COLS = 128                                        # csrc/head.hip: kHeadMaxFm
    # the side options' limits live beside their refusals (branches.py); the names read outside the package
    CROSS_MODELS = SIDE_MODELS
    AFM_MAX_ATT, AFM_MAX_FIELDS = branches.AFM_MAX_ATT, branches.AFM_MAX_FIELDS
    CCPM_MAX_LAYERS, CCPM_MAX_FILTERS, CCPM_MAX_FIELDS = branches.CCPM_MAX_LAYERS, branches.CCPM_MAX_FILTERS, branches.CCPM_MAX_FIELDS
    CIN_MAX_LAYERS, CIN_MAX_MAPS, CIN_MAX_FIELDS, CIN_MAX_WEIGHTS = branches.CIN_MAX_LAYERS, branches.CIN_MAX_MAPS, branches.CIN_MAX_FIELDS, branches.CIN_MAX_WEIGHTS

    def __init__(self, model, C=13, V=0, S=26, E=16, cate_index_size=1000, hidden=(400, 400, 400),
                 multi_ranges=(), Fw=0, lr=0.001, l2=1e-5, decay_steps=10000000, decay_rate=0.9,
                 beta1=0.9, beta2=0.999, eps=1e-8, logloss_eps=1e-7, tower="f32", dropout_keep_deep=None,
                 dropout_keep_fm=None, pos_weight=1.0, cross_layers=0, wide_optimizer="adam", wide_lr=None,
                 wide_l1=0.0, wide_l2=0.0, afm_attention=0, pnn=None, batch_norm=False, bn_eps=1e-5, bn_momentum=0.1,
                 bi_interaction=False, ccpm_filters=(), cin_layers=(), autoint_layers=0, autoint_heads=2,
                 autoint_dim=16):
        given = locals()      # the keywords by name, for the side options' table
        if model not in FAMILIES:
            raise ValueError("unsupported model %r" % model)
        if wide_optimizer not in ("adam", "ftrl"):
            raise ValueError("wide_optimizer must be 'adam' or 'ftrl', got %r" % (wide_optimizer,))
        if wide_optimizer == "ftrl" and model != "wdl":
            raise ValueError("wide_optimizer='ftrl': only wdl has wide weights, not %s" % model)
        for k, v, ok in (("wide_lr", wide_lr, lambda x: x > 0.0), ("wide_l1", wide_l1, lambda x: x >= 0.0),
                         ("wide_l2", wide_l2, lambda x: x >= 0.0)):
            if v is not None and not (math.isfinite(float(v)) and ok(float(v))):
                raise ValueError("wide_optimizer: %s must be finite and %s 0, got %r"
                                 % (k, ">" if k == "wide_lr" else ">=", v))
        self.wide_optimizer = wide_optimizer
        self.wide_lr = None if wide_lr is None else float(wide_lr)
        self.wide_l1, self.wide_l2 = float(wide_l1), float(wide_l2)
        for b in BRANCHES:      # the side options' keywords, as their descriptors coerce them
            for k, v in zip(b.keywords, b.coerce(*(given[k] for k in b.keywords))):
                setattr(self, k, v)
        pos_weight = float(pos_weight)
        if not (math.isfinite(pos_weight) and pos_weight > 0.0):
            raise ValueError("pos_weight must be finite and > 0, got %r" % (pos_weight,))
        self.pos_weight = pos_weight
        fam = FAMILIES[model]
        self.model = model
        self.cont_mode = fam["cont"]
        self.C = C if fam["cont"] else 0          # cate algs have no cont_feats (data_loader.py:8)
        self.V = 0 if model == "wdl" else V
        self.S, self.E = S, E
        self.cate_index_size = cate_index_size
        self.hidden = list(hidden)
        self.multi_ranges = [list(r) for r in multi_ranges] if fam["multi"] else []
        self.Fw = Fw
        # the lookup kernels' field limits (csrc/embed.hip check_layout, launch_embed_fwd), which the
        # library itself reports only at the first launch
        if self.fm_cont and self.C > self.MAX_FM_CONT:
            raise ValueError("C=%d: at most %d FM cont fields (the embedding backward keeps their rows in "
                             "registers)" % (self.C, self.MAX_FM_CONT))
        slots = (self.C if self.fm_cont else 0) + 2 * S if self.fm else S
        if slots > self.MAX_SLOTS:
            raise ValueError("too many fields per sample for the embedding lookup: %d slots (%s), at most %d"
                             % (slots, "FM cont + 2 * single cate" if self.fm else "single cate", self.MAX_SLOTS))
        if self.fm_cols > self.MAX_FM_COLS:
            raise ValueError("too many FM columns for the output layer: %d FM fields + E=%d second-order columns "
                             "= %d, at most %d" % (self.F, E, self.fm_cols, self.MAX_FM_COLS))
        self.lr, self.l2 = lr, l2
        self.decay_steps, self.decay_rate = decay_steps, decay_rate
        self.beta1, self.beta2, self.eps, self.logloss_eps = beta1, beta2, eps, logloss_eps
        if tower not in ("f32", "bf16"):
            raise ValueError("tower must be 'f32' or 'bf16'")
        self.tower = tower      # bf16: the deep tower's GEMMs on bf16 MFMA (config C5), fp32 master weights
        if dropout_keep_deep is not None:
            keep = [float(k) for k in dropout_keep_deep]
            n = len(self.hidden) + 1
            if len(keep) < n:
                raise ValueError("dropout_keep_deep needs %d values (the tower input + %d layers), got %d"
                                 % (n, n - 1, len(keep)))
            keep = keep[:n]
            if not all(0.0 < k <= 1.0 for k in keep):
                raise ValueError("dropout_keep_deep values must lie in (0, 1], got %r" % (keep,))
            dropout_keep_deep = keep
        self.dropout_keep_deep = dropout_keep_deep
        if dropout_keep_fm is not None:
            keep = [float(k) for k in dropout_keep_fm]
            if len(keep) < 2:
                raise ValueError("dropout_keep_fm needs 2 values (first order, second order), got %d" % len(keep))
            keep = keep[:2]
            if not all(0.0 < k <= 1.0 for k in keep):
                raise ValueError("dropout_keep_fm values must lie in (0, 1], got %r" % (keep,))
            dropout_keep_fm = keep if fam["fm"] and any(k < 1.0 for k in keep) else None
        self.dropout_keep_fm = dropout_keep_fm
        for b in BRANCHES:
            values = b.values(self)
            if not values[0]:
                continue
            if b.phrases:
                self._check_side_option(b.name, *b.phrases)
            why = b.refusal and b.refusal(self.afm_fields, self.E, self.deep_in, *values)
            if why:
                raise ValueError("%s: %s" % (b.name, why))
        if self.pnn and self.dropout and self.dropout[1] < 1.0:
            raise ValueError("pnn: not supported with dropout on the first layer's output "
                             "(dropout_keep_deep[1] < 1: that layer's ReLU and dropout live in the GEMM "
                             "epilogue the product layer replaces)")
        if self.batch_norm:
            if tower == "bf16":
                raise ValueError("batch_norm: not supported with tower='bf16' (the normalisation finishes the "
                                 "f32 tower's stored pre-activations)")
            if self.dropout and any(k < 1.0 for k in self.dropout[1:]):
                raise ValueError("batch_norm: not supported with dropout on a hidden layer's output "
                                 "(dropout_keep_deep[l + 1] < 1: that layer's ReLU and dropout live in the GEMM "
                                 "epilogue the normalisation replaces)")
            if self.pnn:
                raise ValueError("batch_norm: not supported together with pnn (both finish layer 0's stored "
                                 "pre-activation in place)")

    def _check_side_option(self, opt, joins, reads_f32, reads_undropped):
        """The refusals every option on the tower input of the SIDE_MODELS shares, in that option's words."""
        if self.model not in SIDE_MODELS:
            raise ValueError("%s: %s the tower of %s only, not %s"
                             % (opt, joins, ", ".join(SIDE_MODELS), self.model))
        if self.tower == "bf16":
            raise ValueError("%s: not supported with tower='bf16' (%s)" % (opt, reads_f32))
        if self.dropout and self.dropout[0] < 1.0:
            raise ValueError("%s: not supported with tower-input dropout (dropout_keep_deep[0] < 1 rewrites x0 in "
                             "place; %s)" % (opt, reads_undropped))

    @property
    def afm_fields(self):
        """The fields the attentional interactions pair (and the product layer mixes, the
        Bi-Interaction pools and the CCPM branch convolves): single-valued, then pooled slots."""
        return self.S + self.M

    def ccpm_dims(self):
        """[(H, W, C)] of the CCPM branch's input map and of every pooled map."""
        out = [(self.E, self.afm_fields, 1)]
        for c in self.ccpm_filters:
            out.append((out[-1][0] // 2, out[-1][1] // 2, c))
        return out

    def cin_weights(self):
        """The CIN's layer weights: sum_k H_k H_{k-1} F, H_0 = F."""
        return branches.cin_weights(self.afm_fields, self.cin_layers)

    @property
    def ftrl_lr(self):
        """FTRL's constant learning rate: wide_lr, or the model's (undecayed) learning rate."""
        return float(self.lr if self.wide_lr is None else self.wide_lr)

    @property
    def dropout(self):
        """The keep probabilities [tower input, layer 0, ...] when any is below 1, else None."""
        k = self.dropout_keep_deep
        return k if k is not None and any(x < 1.0 for x in k) else None

    @property
    def fm(self):
        return FAMILIES[self.model]["fm"]

    @property
    def fm_cont(self):
        """The cont fields are FM fields (deepfm_pipeline, deepfm_multi, deepfm)."""
        return self.fm and self.cont_mode in ("first", "last", "field") and self.C > 0

    @property
    def fm_cont_offset(self):
        """Table row of FM cont field 0."""
        return {"last": self.cate_index_size, "field": self.S}.get(self.cont_mode, 0)

    @property
    def zero_row0(self):
        """Row 0 is forced to zeros every step (deepfm_pipeline.py:83-86); wdl.py:44,
        deepfm.py:58-60 and dnn.py:49-52 have no zero row."""
        return self.model not in ("wdl", "deepfm", "dnn")

    @property
    def xavier_table(self):
        """glorot-uniform table named weight_mat (wdl.py:44-47, dnn.py:49-52)."""
        return self.model in ("wdl", "dnn")

    @property
    def table_key(self):
        return "weight_mat" if self.xavier_table else "feats_emb"

    @property
    def first_key(self):
        return "feats" if self.model == "deepfm" else "fm_first_order_emb"   # deepfm.py:60

    @property
    def sparse_table(self):
        """The table (and first-order) Variables are read by tf.nn.embedding_lookup directly,
        so TF updates them with Adam's sparse-apply form (Adam._apply_sparse_shared): wdl.py:44-47,
        132 weight_mat, deepfm.py:57-60,78,85,98 feats_emb / feats, dnn.py:49-54 weight_mat.  The
        pipeline models concat a zero row 0 first (deepfm_pipeline.py:83-86), which densifies the
        gradient: ApplyAdam."""
        return self.model in ("wdl", "deepfm", "dnn")

    @property
    def hidden_reg(self):
        """Regulariser on the hidden weight matrices: wdl.py:272-275 L2, dnn.py:88-90 L1."""
        return {"wdl": "l2", "dnn": "l1"}.get(self.model)

    @property
    def head_l2(self):
        """L2 on the output weights (deepfm_pipeline.py:183, dnn_pipeline.py:131); dnn.py has none."""
        return self.model != "dnn"

    def head_ref_index(self):
        """Reference index of each internal head weight (FM fields internally [cont | cate |
        pooled]; deepfm.py:70-71 orders its FM fields [cate | cont])."""
        n = self.fm_cols + self.hidden[-1] + 1
        idx = np.arange(n)
        if self.model == "deepfm" and self.C:
            C, S = self.C, self.S
            idx[:C] = S + np.arange(C)
            idx[C:C + S] = np.arange(S)
        return idx

    @property
    def fm_cate_offset(self):
        """Added to a cate id for its FM row (deepfm_pipeline.py:89); the deep row is the raw id."""
        return self.C if self.cont_mode == "first" and self.fm else 0

    @property
    def M(self):
        return len(self.multi_ranges)

    @property
    def multi_width(self):
        return sum(e - s for s, e, *_ in self.multi_ranges)

    @property
    def n_rows(self):
        if self.fm_cont:      # deepfm_pipeline.py:77 / deepfm_multi.py:125: cate_index_size + C
            return self.C + self.cate_index_size
        return self.cate_index_size

    @property
    def deep_in(self):
        return self.S * self.E + self.M * self.E + self.C + self.V + (self.E if self.bi_interaction else 0)

    @property
    def F(self):
        """FM fields: [cont (fm_cont) | single cate | pooled slots]."""
        if not self.fm:
            return 0
        return (self.C if self.fm_cont else 0) + self.S + self.M

    @property
    def fm_cols(self):
        return self.F + self.E if self.fm else 0

    @property
    def cate_ld(self):
        return self.S + self.multi_width

    def check_deep0(self, P):
        """Refuses reference-layout parameters whose deep_0 has another input width: the one shape
        bi_interaction changes, so parameters of the other setting do not load."""
        rows = np.shape(P["deep_0"])[0]
        if rows != self.deep_in:
            raise ValueError("deep_0 has %d rows for %d tower-input columns: with bi_interaction=%s the tower "
                             "input %s the %d Bi-Interaction columns, and parameters of the other setting do "
                             "not load" % (rows, self.deep_in, self.bi_interaction,
                                           "holds" if self.bi_interaction else "does not hold", self.E))

    def x0_ref_rows(self):
        """Reference row of W_0 for each internal x0 column < deep_in.  Every pipeline-style
        model concatenates its deep input as [cont, vector, single cate, pooled]
        (deepfm_pipeline.py:123, deepfm_multi.py:188, dnn_multi.py:106, deepfm_multi_cate.py:169,
        wdl.py:179); absent parts are empty."""
        S, E, M, C, V = self.S, self.E, self.M, self.C, self.V
        cat = np.arange(S * E) + C + V
        pool = np.arange(M * E) + C + V + S * E
        cont = np.arange(C)
        vec = np.arange(V) + C
        # bi_interaction: the reference order ends with q; internally q follows the fields it pools
        bi = np.arange(E if self.bi_interaction else 0) + C + V + (S + M) * E
        return np.concatenate([cat, pool, bi, cont, vec])


def _root_to_v(s):
    """Device root state s = sqrt(v) (a tensor) -> TF's v, fl(s * s), as host numpy."""
    a = s.cpu().numpy().astype(np.float64)
    return (a * a).astype(np.float32)


def _v_to_root(v):
    """TF's v (array-like) -> the root state fl(sqrt(v)), host numpy f32."""
    return np.sqrt(np.ascontiguousarray(v, np.float64)).astype(np.float32)

class CTREngine:
    def __init__(self, spec, max_batch, device="cuda", seed=2019, init="device", bwd="atomic",
                 table_rows=None, adam="dense", hist_len=4096, rec_stash=True, gemm="s3", sample_weight=False):
        # sample weights (tf.losses.log_loss's weights=): on with sample_weight (the
        # batch's "weight" entry) or with ModelSpec.pos_weight != 1
        self.weighted = bool(sample_weight) or spec.pos_weight != 1.0
        if self.weighted and type(self) is not CTREngine:
            raise ValueError("sample_weight / pos_weight: not supported by %s (the loss normaliser, the batch's "
                             "nonzero-weight count, would need an all-reduce across the ranks)" % type(self).__name__)
        if spec.wide_optimizer == "ftrl" and type(self) is not CTREngine:
            raise ValueError("wide_optimizer='ftrl': not supported by %s (its owner-side wide update is Adam's)"
                             % type(self).__name__)
        if not torch.cuda.is_available():
            raise _lib.DLError("CTREngine needs a HIP device (no CPU fallback)")
        _lib.lib()
        self.spec = sp = spec
        # dropout of the deep tower (ModelSpec.dropout_keep_deep): in the s3 epilogues, whose
        # combined (sign & keep) bitmask the dX GEMMs read; the mask's seed is the engine's
        self.seed = int(seed)
        self.drop = sp.dropout
        if self.drop:
            if sp.tower == "bf16":
                raise ValueError("dropout_keep_deep: not supported with tower='bf16' (the dropout epilogues are "
                                 "the f32 s3 tower's)")
            if gemm == "f32":
                raise ValueError("dropout_keep_deep: not supported with gemm='f32' (the dropout epilogues are "
                                 "the s3 GEMMs')")
            if type(self) is not CTREngine:
                raise ValueError("dropout_keep_deep: not supported by %s (the mask is indexed by the local "
                                 "row number; a sharded batch needs global rows)" % type(self).__name__)
            if sp.fm and sp.M and self.drop[0] < 1.0:
                raise ValueError("dropout_keep_deep: input dropout (keep[0] < 1) is not supported for FM models "
                                 "with multi-hot slots (their FM backward reads the pooled vectors from x0, "
                                 "which the input dropout overwrites)")
        # dropout of the FM part (ModelSpec.dropout_keep_fm): drawn by the head, which leaves the keep
        # bits in fm_keep for the FM backward twins (include/dlamd.h "Dropout")
        self.fmdrop = sp.dropout_keep_fm
        if self.fmdrop and type(self) is not CTREngine:
            raise ValueError("dropout_keep_fm: not supported by %s (the mask is indexed by the local "
                             "row number; a sharded batch needs global rows)" % type(self).__name__)
        if type(self) is not CTREngine:      # the side options only this class's own step carries
            branches.unsupported(sp, type(self).__name__)
        self.dev = torch.device(device)
        self.B = max_batch
        # set later: predict's planes (flush(planes=True)) and the step they were written at,
        # fused_gather_tab's offsets, the prefetch's side stream and buffer sets (_enable_slots)
        self.p_plane = self.w1_plane = self.gtab = self.side = self._slots = None
        self.planes_step = -1
        self._cur = 0      # the buffer set in use
        self._pfq = []     # pending prefetches, oldest first: (set, B, ready event, batch)
        self._pf = None    # the oldest pending prefetch (_pfq[0])
        dev = self.dev
        z = lambda *s, dt=F32: torch.zeros(*s, dtype=dt, device=dev)
        E, S, M = sp.E, sp.S, sp.M
        N = sp.n_rows
        self.N = N
        # ---- layout
        self.cat_col = 0
        self.pool_col = S * E
        # Bi-Interaction pooling (ModelSpec.bi_interaction, csrc/bi.hip): q in the E columns after the
        # last field, before cont and vector, so [fields | q] is one range of x0 and of dx0 (layer 0's
        # dX GEMM covers dq by the wider dx_cols); nothing else is allocated
        self.bi = sp.bi_interaction
        self.bi_col = (S + M) * E
        self.cont_col = (S + M) * E + (E if self.bi else 0)
        self.vec_col = self.cont_col + sp.C
        self.D0 = sp.deep_in
        dims = [self.D0] + sp.hidden
        self.in_ld = [_ru(d + 1, 16) for d in dims[:-1]]
        self.out_ld = [_ru(h, 16) for h in sp.hidden]
        self.h_ld = [_ru(h + 1, 16) for h in sp.hidden]
        self.fm_ld = _ru(max(sp.fm_cols, 1), 4)
        self.dx_cols = (S + M) * E + (E if self.bi else 0)
        self.dx_ld = _ru(max(self.dx_cols, 4), 4)
        # ---- parameters + Adam state
        rows_pad = _ru(table_rows if table_rows is not None else N, 16)
        self.rows_pad = rows_pad
        if adam not in ("dense", "lazy"):
            raise ValueError("adam must be 'dense' or 'lazy'")
        self.lazy = adam == "lazy"
        if self.lazy:
            # row records + lazy-exact Adam (rec.hip); needs the batch index (with multi-hot
            # slots it also indexes every multi-hot id position: pooling reads caught-up rows)
            bwd = "sorted"
            self.rec_ld = _ru(3 * E + 4, 32)
            self.rec = z(rows_pad, self.rec_ld)
            self.hist_len = hist_len
            self.hist = z(hist_len)
            self.n_rep = sp.C if sp.fm_cont else 0     # FM cont-field rows (replicated, hot)
            R = max(self.n_rep, 1)
            self.g_rep, self.g1_rep = z(_ru(R * E, 4)), z(_ru(R, 4))
            self.rep_touched = z(_ru(R, 16), dt=torch.uint8)
            self.since_flush = 0
            self.table = self.tm = self.tv = self.tg = self.touched = None
            self.first = self.fmm = self.fmv = self.fmg = None
        else:
            self.table = z(rows_pad, E)
            self.tm, self.tv, self.tg = z(rows_pad, E), z(rows_pad, E), z(rows_pad, E)
            self.touched = z(rows_pad, dt=torch.uint8)
            if sp.fm:
                self.first = z(rows_pad)
                self.fmm, self.fmv, self.fmg = z(rows_pad), z(rows_pad), z(rows_pad)
            else:
                self.first = self.fmm = self.fmv = self.fmg = None
        self.W = [z(self.in_ld[l], self.out_ld[l]) for l in range(len(sp.hidden))]
        self.Wm = [torch.zeros_like(w) for w in self.W]
        self.Wv = [torch.zeros_like(w) for w in self.W]
        self.Wt = z(max(o * i for o, i in zip(self.out_ld, self.in_ld)))   # W_l^T scratch for dX
        # fp32 tower products on the bf16 matrix cores through the exact three-plane split
        # (gemm_s3.hip, f32 accuracy): bf16 planes of W (the dX operand, [in][out]) and of W^T
        # (the forward operand, [out][in]), refreshed after every update of W
        if gemm not in ("s3", "f32"):
            raise ValueError("gemm must be 's3' or 'f32'")
        self.s3 = gemm == "s3" and sp.tower == "f32"
        if self.s3:
            zp = lambda n: torch.zeros(n, dtype=torch.int16, device=dev)
            self.Wp = [zp(3 * self.in_ld[l] * self.out_ld[l]) for l in range(len(sp.hidden))]
            self.WTp = [zp(3 * self.out_ld[l] * self.in_ld[l]) for l in range(len(sp.hidden))]
        H = sp.hidden[-1]
        self.head_n = sp.fm_cols + H + 1
        self.w_head = z(_ru(self.head_n, 4))
        self.hm, self.hv = torch.zeros_like(self.w_head), torch.zeros_like(self.w_head)
        self.w_head_prev = torch.zeros_like(self.w_head)
        self.opt = z(_lib.OPT_LEN)   # include/dlamd.h: Adam scalars, per-step sums, status word
        self.opt[:8].copy_(torch.tensor([sp.beta1, sp.beta2, sp.lr, 0.0, sp.beta1, sp.beta2, sp.eps, 0.0]))
        self.wdl = sp.model == "wdl"
        # FTRL-proximal on wdl_weights (ModelSpec.wide_optimizer, wide.hip): wm / wv (the records'
        # second and third floats) hold FTRL's z and n; no flush, no wide L2 loss term
        self.ftrl = sp.wide_optimizer == "ftrl"
        self.w_rows = 0
        if self.wdl:   # wdl_weights [N + H] (deep-output rows alias wide ids, wdl.py:241-248) + bias
            self.w_rows = N + sp.hidden[-1]
            wr = _ru(self.w_rows, 16)
            self.ww, self.wm, self.wv = z(wr), z(wr), z(wr)
            # wide gradient: int64 fixed point (deterministic integer atomics, head.hip)
            self.wg = z(wr, dt=torch.int64)
            self.w_touched = z(wr, dt=torch.uint8)
            self.wb, self.wbm, self.wbv = z(4), z(4), z(4)
        # wide_lazy (single-GPU wdl with lazy tables): wdl_weights as {w, m, v, stamp} records
        # with lazy-exact Adam (wide.hip): the batch's unique wide ids indexed, gathered caught
        # up into the head's compact local table [— (Fw) | deep-output rows | unique rows], and
        # only those rows (and the H deep-output rows) updated — in place of the dense L2 sweep
        # over all N + H rows (wdl.py:270-271); bit-identical to it.  The table ids and the wide ids
        # go through ONE index build (dl_index_build_pair): the table's index arrays hold both sets'
        # sorted references and unique rows, the wide set's own arrays (widx_*) are split out of them
        self.wide_lazy = self.wdl and self.lazy and type(self) is CTREngine
        self.wide_flushes = self.wide_lazy and not self.ftrl   # Adam's records lag and need catching up
        if self.wide_lazy:
            Fw, Hh, Bm = sp.Fw, sp.hidden[-1], max_batch
            nw = Bm * Fw
            self.wrec = z(_ru(self.w_rows, 16), 4)    # {w, m, v, stamp} (wide.hip)
            self.wloc = z(_ru(Fw + Hh + nw, 4))
            self.wgloc = z(Fw + Hh + nw, dt=torch.int64)
            self.wstash = z(max(nw, 1), 4)
            self.wdmark = z(_ru(Hh, 16), dt=torch.uint8)
            self.wlong = z(nw + 1, dt=torch.int32)   # dl_wide_seg_grad's hot-row list
            # the update kernels' per-block partial sums of the touched rows' L2 term
            self.wsq_part = z(max(1, int(_lib.lib().dl_wide_update_blocks(nw, Hh))))
            self.wsq = z(2, dt=torch.int64)      # L2 term of the rows the last step left (a flush; fixed point)
            self._wsq_step = -1
            # the running loss's wide L2 term (loss_sum_begin / loss_sum_end): per-block slots the
            # update and flush kernels add to, and each unique row's replayed steps' w^2 (gather)
            self.wacc = z(_lib.LOSS_ACC_SLOTS, dt=torch.float64)
            self.wrep = z(max(nw, 1))
            self.in_wide_loc = z(Bm, Fw, dt=torch.int64)
            self.widx_refs, self.widx_uniq = (z(max(nw, 1), dt=torch.int32) for _ in range(2))
            self.widx_off = z(nw + 1, dt=torch.int32)
            self.widx_n = z(4, dt=torch.int32)
            self.winv = z(max(nw, 1), dt=torch.int32)
            WL = _lib.EmbLayout()
            WL.n_rows = self.w_rows
            WL.batch = Bm
            WL.emb_dim = sp.E
            WL.cate_fields = Fw
            WL.cate_ld = max(Fw, 1)
            WL.use_fm = 0
            WL.zero_row0 = 0
            self.wlayout = WL
        self.err = z(4, dt=torch.int32)       # the batch's id-validation word (per buffer set)
        # batches prefetched ahead (train_step(next_batch=[...])): buffer sets = pf_depth + 1
        self.pf_depth = int(os.environ.get("DLAMD_PF_DEPTH", "1")) if type(self) is CTREngine else 1
        # running loss of a training loop (dl_loss_accumulate, every step inside its graph):
        # [sum of data terms, sum of regulariser terms, steps]
        self.loss_acc = z(4, dt=torch.float64)
        # table update form (TF: ApplyAdam, or the sparse-apply form for direct lookups)
        self.rec_flags = (_lib.REC_FIRST if sp.fm else 0) | (_lib.REC_SPARSE_ADAM if sp.sparse_table else 0)
        self.rows_sparse = _lib.ROWS_SPARSE_ADAM if sp.sparse_table else 0
        self._status_q = []
        self._status_host = None
        self.host_wait = 0.0
        # DLAMD_STATUS_RING=1: the step's last kernel writes its status into pinned host memory
        # (dl_loss_accumulate's ring) instead of a device-to-host copy after each step
        self._ring = None
        if os.environ.get("DLAMD_STATUS_RING", "1") == "1" and type(self) is CTREngine:
            self._ring = torch.zeros(8, dtype=torch.int32, pin_memory=True)
            self._ring_np = self._ring.numpy()
            self._ring_sent = None
        # ---- activations / workspaces
        B = max_batch
        self.x0 = z(B, self.in_ld[0])
        self.x0[:, self.D0] = 1.0
        self.h = []
        for l, hdim in enumerate(sp.hidden):
            t = z(B, self.h_ld[l])
            t[:, hdim] = 1.0
            self.h.append(t)
        self.dh = [z(B, self.h_ld[l]) for l in range(len(sp.hidden))]
        # the forward's ReLU sign bitmasks (s3 tower; dl_gemm_s3_nt_bits): the dX ReluGrad
        # epilogue reads 2 bytes per 16 columns instead of the f32 activations
        self.hbits_ld = [_ru(-(-h // 16), 32) for h in sp.hidden]
        self.hbits = [z(B, self.hbits_ld[l], dt=torch.int16) for l in range(len(sp.hidden) - 1)] if self.s3 else []
        self.bf = sp.tower == "bf16"
        # bf16 tower without pooled fields: the embedding forward writes the bf16 x0 itself
        self.x0_direct = self.bf and not sp.M
        if self.bf:
            # bf16 tower operands: x0 and hidden activations (bias ones columns included),
            # gradients, and bf16 copies of the fp32 master weights (refreshed after each update)
            zb = lambda *sh: torch.zeros(*sh, dtype=torch.bfloat16, device=dev)
            self.x0b = zb(B, self.in_ld[0])
            self.x0b[:, self.D0] = 1.0
            self.hb = []
            for l, hdim in enumerate(sp.hidden[:-1]):
                t = zb(B, self.h_ld[l])
                t[:, hdim] = 1.0
                self.hb.append(t)
            self.dhb = [zb(B, self.h_ld[l]) for l in range(len(sp.hidden))]
            self.Wb = [zb(self.in_ld[l], self.out_ld[l]) for l in range(len(sp.hidden))]
            # W^T (k-contiguous) for the forward product; dW reads the batch-major X and dY
            # directly (transposing LDS reads in the kernel), so there are no X^T / dY^T copies
            self.WbT = [zb(self.out_ld[l], self.in_ld[l]) for l in range(len(sp.hidden))]
        self.dx0 = z(B, self.dx_ld)
        self.fm_out = z(B, self.fm_ld)
        self.fm_sum = z(B, E)
        if self.fmdrop:
            # the keep bits of a sample's FM columns, two words (bit c of word k: column 64 k + c)
            self.fm_keep = torch.zeros(B, 2, dtype=torch.int64, device=dev)
            self.fm_drop_desc = _lib.FmDrop(fm_keep=self.fm_keep.data_ptr(), inv1=self._keep_inv(self.fmdrop[0]),
                                            inv2=self._keep_inv(self.fmdrop[1]))
        self.score, self.z, self.dz = z(B), z(B), z(B)
        # the side options (branches.py), each under its descriptor's key: the enabled ones' dense parameter
        # vectors with their Adam moments and the backward's per-block partial sums (param_groups.py), in the order
        # of their Adam launches, and the logit chain: per member its labels and entry points, its own leading
        # arguments, its forward's private state and its logit z_<key> [B], every logit with the earlier ones
        # already added, so the last is the head's one z_extra
        self.groups, self.chain = {}, []
        for b in BRANCHES:
            on = getattr(sp, b.name)
            setattr(self, b.key, on)
            if not on:
                continue
            if b.ckpt_keys:
                n, pack, unpack = b.layout(sp)
                reg = dict(reg=(sp.l2, b.reg(sp), self.opt[8:])) if b.reg else {}
                self.groups[b.key] = ParamGroup(b.key, n, "dl_%s_grid" % b.key, B, dev, pack, unpack, b.ckpt_keys, **reg)
            if b.lead:
                self.chain.append(SimpleNamespace(
                    fwd=(b.key + "_fwd", "dl_%s_fwd" % b.key), bwd=(b.key + "_bwd", "dl_%s_bwd" % b.key),
                    lead=b.lead(sp), whole_x0=b.whole_x0, g=self.groups[b.key],
                    state=(z(*b.state(sp, B)),) if b.state else (), z=z(B)))
        # the options that read x0's deep columns (all on the tower input)
        self.reads_x0 = any(getattr(sp, b.name) for b in BRANCHES if b.phrases)
        # batch normalisation (ModelSpec.batch_norm, csrc/bn.hip), per hidden layer: [gamma | beta] as a
        # group of its own (no regulariser), [running_mean | running_var], the step's [mu_hi | mu_lo |
        # invstd] and xhat [B, h_ld]; the statistics' partials and the merged backward sums are consumed at
        # once and shared by the layers
        self.bn_groups = []
        if self.bn:
            dp = [_ru(h, 16) for h in sp.hidden]
            for l, h in enumerate(sp.hidden):
                g = ParamGroup("bn_l%d" % l, 2 * h, "dl_bn_grid", B, dev, partial(bn_pack, l=l, D=h),
                               partial(bn_unpack, l=l, D=h), ("adam/bn_m%d" % l, "adam/bn_v%d" % l))
                g.w[:h] = 1.0
                self.bn_groups.append(g)
            self.bn_run = [z(2, h) for h in sp.hidden]
            for r in self.bn_run:
                r[1] = 1.0
            self.bn_stat = [z(3 * d) for d in dp]
            self.hx = [z(B, self.h_ld[l]) for l in range(len(sp.hidden))]
            self.bn_ws = z(max(call_int("dl_bn_ws_floats", B, h) for h in sp.hidden))
            self.bn_sums = z(2 * max(dp))
        self.head_grid ="dl_wdl_head_grid" if self.wdl else "dl_head_grid"   # slab rows per batch size
        self.head_blocks = call_int(self.head_grid, B)
        self.head_slab = z(self.head_blocks, sp.fm_cols + H + 2)
        self.in_wide = z(B, max(sp.Fw, 1), dt=torch.int64)
        # split-K slabs of the weight gradients: the double-buffered s3 TN kernel (one block per
        # CU, 2 column tiles) runs best at 32 (scripts/s3_bench.py: 147 vs 152 us at 64)
        # (the bf16 tower's ring kernel, one 144 x 400 block per CU, takes up to 96: _bf16_dw_splits)
        dflt = 32 if self.s3 else 96 if self.bf else 64
        self.splits = max(1, min(int(os.environ.get("DLAMD_DW_SPLITS", dflt)), B // (512 if self.bf else 1024)))
        self.dw_splits = self._dw_splits(B, fixed="DLAMD_DW_SPLITS" in os.environ)
        # sized for the cap: a smaller batch may choose more splits than the largest one did
        # (one slab set per layer when the dense Adams run as one launch after the backward's
        # GEMMs, _adam_fused: each layer's slabs must survive until then)
        per = [self.splits * i * o for i, o in zip(self.in_ld, self.out_ld)]
        self.w_slab = z(sum(per) if self._adam_fused() else max(per))
        offs = np.cumsum([0] + per)
        self.w_slabs = [self.w_slab[offs[l]:offs[l + 1]] if self._adam_fused() else self.w_slab
                        for l in range(len(per))]
        self.layout = self._layout(B)
        self.bwd_blocks = _lib.lib().dl_embed_bwd_grid(C_ref(self.layout))
        self.cont_slab = z(max(1, self.bwd_blocks * sp.C * (E + 1)))
        self.fm_pool_col = sp.F - M      # head column of the first pooled first-order output
        if M:
            self.slot_start = torch.tensor([r[0] for r in sp.multi_ranges], dtype=torch.int32, device=dev)
            self.slot_end = torch.tensor([r[1] for r in sp.multi_ranges], dtype=torch.int32, device=dev)
            self.cnt_emb, self.cnt_first = z(B, M), z(B, M)
            if self.lazy:
                # per (sample, slot): the slot gradient (E floats) and the first-order one at
                # column E of a row padded to whole 128-B lines (one line fetch per multi-hot
                # reference in the backward instead of two: dl_pool_desc.g_pitch)
                gp = _ru(E + 1, 32)
                self.g_pool = z(B, M, gp)
                self.g1_pool = self.g_pool.view(-1)[E:]
                self.pool_desc = _lib.PoolDesc(
                    slot_start=self.slot_start.data_ptr(), slot_end=self.slot_end.data_ptr(), n_slots=M,
                    fm_col=self.fm_pool_col, dx0_pool_col=S * E, g_pitch=gp, x0=self.x0.data_ptr(),
                    cnt_emb=self.cnt_emb.data_ptr(), cnt_first=self.cnt_first.data_ptr(),
                    g_pool=self.g_pool.data_ptr(), g1_pool=self.g1_pool.data_ptr())
        # batch reference index (deterministic backward)
        self.bwd = bwd
        self.n_slot = (S if sp.fm else 0) + S + (sp.multi_width if self.lazy else 0)
        self.n_refs = B * self.n_slot
        if bwd == "sorted":
            cap = self.n_refs + (B * sp.Fw if self.wide_lazy else 0)   # the pair build's wide references
            wsb = _lib.lib().dl_index_workspace_bytes(max(1, cap))
            self.idx_ws = z(wsb, dt=torch.uint8)
            self.idx_keys = z(cap, dt=torch.int32)
            self.idx_refs = z(cap, dt=torch.int32)
            self.idx_uniq = z(cap, dt=torch.int32)
            self.idx_off = z(cap + 1, dt=torch.int32)
            self.idx_n = z(4, dt=torch.int32)
            self.idx_inv = z(cap, dt=torch.int32) if self.lazy else None
        if self.lazy:
            self.rows_u = z(self.n_rep + self.n_refs, E)
            self.rows_u1 = z(self.n_rep + self.n_refs)
            # rec_stash: the gather also stashes the caught-up moments for the backward's update.
            # Off by default — re-reading the record in the backward measured faster on both
            # kernels (gather 328 -> 232 us, backward 505 -> 447 us at C2; profiles/r01l).
            self.mv_u = z(self.n_rep + self.n_refs, int(_lib.lib().dl_rec_stash_floats(E))) if rec_stash else None
            # hot rows' chunked segment sums (dl_rec_bwd_adam: Zipf rows over many blocks)
            self.hot_ws = z(int(_lib.lib().dl_rec_bwd_workspace_bytes(self.n_refs, E)), dt=torch.uint8)
        # static input slots (graph capture reads from these)
        self.in_label = z(B)
        self.in_cont = z(B, max(sp.C, 1))
        self.in_vec = z(B, max(sp.V, 1))
        self.in_cate = z(B, max(sp.cate_ld, 1), dt=torch.int64)
        if self.weighted:
            # the batch's weights, its effective weights and {inv_norm, N_nz} (dl_weight_norm, in _pre):
            # per buffer set, as the labels they belong to
            self.in_weight, self.w_eff, self.norm = z(B), z(B), z(4)
        self.graphs = {}        # (buffer set, batch, not indexed) -> captured step; (set, batch, "pre") -> index build
        # predict on a flushed table reads dense p / first-order planes written by the flush
        # (DLAMD_FLAT_PLANES=0: each reference reads its record's first line instead)
        self.flat_planes = os.environ.get("DLAMD_FLAT_PLANES", "1") != "0"
        self.prof = None
        self.steps = 0
        if init == "device":
            self.init_device(seed)

    # ------------------------------------------------------------------ layout
    def _layout(self, B):
        sp = self.spec
        L = _lib.EmbLayout()
        L.n_rows = self.N
        L.fm_cont_offset = sp.fm_cont_offset                            # deepfm_multi.py:139
        L.fm_cate_offset = sp.fm_cate_offset                            # deepfm_pipeline.py:89
        L.deep_cate_offset = 0                                          # :120 raw ids
        L.batch = B
        L.emb_dim = sp.E
        L.cont_fields = sp.C
        L.vector_size = sp.V
        L.cate_fields = sp.S
        L.cate_ld = sp.cate_ld
        L.fm_cont = 1 if sp.fm_cont else 0
        L.use_fm = 1 if sp.fm else 0
        L.fm_extra = sp.M if sp.fm else 0
        L.zero_row0 = 1 if sp.zero_row0 else 0                         # :83-86 (wdl.py:49: none)
        L.x0_ld = self.in_ld[0]
        L.x0_cont_col = self.cont_col if sp.C else -1
        L.x0_vec_col = self.vec_col if sp.V else -1
        L.x0_cat_col = self.cat_col
        L.x0_pool_col = self.pool_col
        L.fm_ld = self.fm_ld
        L.dx0_ld = self.dx_ld
        L.dx0_cat_col = 0
        L.multi_width = sp.multi_width if self.lazy else 0
        L.cont_rows_compact = 1 if self.lazy else 0     # records: cont rows gathered first into rows_u
        L.x0_bf16 = 1 if self.x0_direct else 0           # bf16 tower: the forward writes x0 as bf16
        return L

    def _flat_layout(self, B):
        """The layout of the dense-table forward over the flushed planes (the replicated FM
        cont rows read from the planes in place, no batch index)."""
        L = self._layout(B)
        L.cont_rows_compact = 0
        L.multi_width = 0
        return L

    # ------------------------------------------------------------------ params
    def init_device(self, seed):
        """Reference initialisers (deepfm_pipeline.py:78-80,131-169): table ~ N(0, 0.01),
        first-order ~ U[0,1), dense weights/biases ~ N(0, glorot) (numpy, seeded)."""
        sp = self.spec
        s = _lib.stream_handle()
        if self.lazy:   # same values as the dense engine: initialise dense, then pack
            self.table = torch.zeros(self.rows_pad, sp.E, device=self.dev)
            self.first = torch.zeros(self.rows_pad, device=self.dev) if sp.fm else None
        if sp.xavier_table:   # xavier_initializer (wdl.py:44-47, dnn.py:49-52): U(-lim, lim), lim = sqrt(6/(N+E))
            lim = math.sqrt(6.0 / (self.N + sp.E))
            call("dl_init_random", ptr(self.table), self.table.numel(), 1, -lim, 2 * lim, seed, 0, s)
        if self.wdl:
            call("dl_init_random", ptr(self.ww), _ru(self.ww.numel(), 4), 0, 0.0,
                 math.sqrt(2.0 / self.w_rows), seed + 3, 0, s)                           # wdl.py:241-244
            self.ww[self.w_rows:].zero_()
            self.wb[0] = float(np.random.default_rng(seed).standard_normal())
            self._ftrl_reset()
        if not sp.xavier_table:
            call("dl_init_random", ptr(self.table), self.table.numel(), 0, 0.0, 0.01, seed, 0, s)
        if self.first is not None:
            call("dl_init_random", ptr(self.first), self.first.numel(), 1, 0.0, 1.0, seed + 1, 0, s)
        if self.lazy:
            self._pack(self.table, self.first)
            self.table = self.first = None
        rng = np.random.default_rng(seed)
        dims = [self.D0] + sp.hidden
        for l in range(len(sp.hidden)):
            g = math.sqrt(2.0 / (dims[l] + dims[l + 1]))
            self._set_layer(l, (rng.standard_normal((dims[l], dims[l + 1])) * g).astype(np.float32),
                            (rng.standard_normal((1, dims[l + 1])) * g).astype(np.float32), ref_order=False)
        H = sp.hidden[-1]
        g = math.sqrt(2.0 / (self.head_n))
        w = np.zeros(self.head_n, np.float32)
        w[:-1] = rng.standard_normal(self.head_n - 1) * g
        w[-1] = rng.standard_normal()
        self.w_head[: self.head_n].copy_(torch.from_numpy(w))
        for b in BRANCHES:      # in the order of the table: rng is consumed branch by branch
            g = self.groups.get(b.key)
            if g is not None:
                g.load(b.init(rng, sp, g.unpack))
        if self.wide_lazy:
            self._wide_pack()
        torch.cuda.synchronize()

    def _set_layer(self, l, W, b, ref_order=True):
        din = W.shape[0]
        Wi = np.zeros((self.in_ld[l], self.out_ld[l]), np.float32)
        if l == 0 and ref_order:
            Wi[:din, : W.shape[1]] = W[self.spec.x0_ref_rows()]
        else:
            Wi[:din, : W.shape[1]] = W
        Wi[din, : W.shape[1]] = b.reshape(-1)
        self.W[l].copy_(torch.from_numpy(Wi))
        self._refresh_wb(l)

    def _refresh_wb(self, l, s=None):
        """The tower's operand copies of the fp32 master weights W_l: bf16 tower, bf16 W and
        W^T; split (s3) GEMMs, the three bf16 planes of W and of W^T."""
        if self.s3:
            s = s if s is not None else _lib.stream_handle()
            i, o = self.in_ld[l], self.out_ld[l]
            call("dl_split3", ptr(self.W[l]), i, o, o, 0, ptr(self.Wp[l]), o, i * o, s)
            call("dl_split3", ptr(self.W[l]), i, o, o, 1, ptr(self.WTp[l]), i, i * o, s)
        if self.bf:
            s = s if s is not None else _lib.stream_handle()
            call("dl_cast_bf16", ptr(self.W[l]), self.in_ld[l], self.out_ld[l], self.out_ld[l], ptr(self.Wb[l]),
                 self.out_ld[l], s)
            call("dl_transpose_bf16", ptr(self.W[l]), 1, self.in_ld[l], self.out_ld[l], self.out_ld[l],
                 ptr(self.WbT[l]), self.in_ld[l], s)

    def load_params(self, P):
        """Inject reference-layout parameters (dict of numpy arrays as in oracle/ctr_ref.py)."""
        sp = self.spec
        N = self.N
        tab = torch.from_numpy(np.ascontiguousarray(P[sp.table_key], np.float32))
        first = (torch.from_numpy(np.ascontiguousarray(P[sp.first_key][:, 0], np.float32))
                 if sp.fm else None)
        if self.lazy:
            self._pack(tab.to(self.dev), first.to(self.dev) if first is not None else None)
        else:
            self.table.zero_()
            self.table[:N].copy_(tab)
            if self.first is not None:
                self.first.zero_()
                self.first[:N].copy_(first)
        sp.check_deep0(P)
        for l in range(len(sp.hidden)):
            self._set_layer(l, P["deep_%d" % l], P["deep_bias_%d" % l])
        if self.bn:
            self._bn_load(P)
        if self.wdl:
            self.ww.zero_()
            self.ww[: self.w_rows].copy_(torch.from_numpy(np.ascontiguousarray(P["wdl_weights"][:, 0], np.float32)))
            self.wb.zero_()
            self.wb[:1].copy_(torch.from_numpy(np.asarray(P["wdl_bias"], np.float32).reshape(-1)))
            self._load_ftrl(P)
            if self.wide_lazy:
                if not self.ftrl:
                    self.wm.zero_()
                    self.wv.zero_()
                self._wide_pack()
            torch.cuda.synchronize()
            return
        if sp.fm:
            w = np.concatenate([P["deep_fm_weight"][:, 0], P["deep_fm_bias"].reshape(-1)]).astype(np.float32)
        else:
            w = np.concatenate([P["deep_res"][:, 0], P["deep_res_bias"].reshape(-1)]).astype(np.float32)
        w = w[sp.head_ref_index()]
        self.w_head.zero_()
        self.w_head[: self.head_n].copy_(torch.from_numpy(w))
        for g in self.groups.values():
            g.load(P)
        torch.cuda.synchronize()

    def _bn_load(self, P):
        """Reference-layout gamma, beta and running statistics of every hidden layer -> the device
        (absent running statistics: torch's initial 0 and 1)."""
        for l, (g, D) in enumerate(zip(self.bn_groups, self.spec.hidden)):
            g.load(P)
            self.bn_run[l].copy_(torch.from_numpy(np.stack([bn_vec(P, l, "running_mean", D, 0.0),
                                                            bn_vec(P, l, "running_var", D, 1.0)])))

    def params(self):
        """Export parameters in the reference layout (numpy)."""
        sp = self.spec
        N = self.N
        if self.lazy:
            self.flush()
            rec = self.rec[:N]
            P = {sp.table_key: rec[:, : sp.E].cpu().numpy()}
            if sp.fm:
                P[sp.first_key] = rec[:, sp.E: sp.E + 1].cpu().numpy()
        else:
            P = {sp.table_key: self.table[:N].cpu().numpy()}
            if self.first is not None:
                P[sp.first_key] = self.first[:N].cpu().numpy()[:, None]
        P.update(self.dense_params())
        return P

    def _dw_splits(self, B, fixed=False):
        """Per-layer split-K slab counts of the weight gradients (fixed: self.splits for all)."""
        base = max(1, min(self.splits, B // (512 if self.bf else 1024)))
        if fixed or not (self.s3 or self.bf):
            return [base] * len(self.spec.hidden)
        if self.bf:
            return [_bf16_dw_splits(i, B, base) for i in self.in_ld]
        return [_s3_dw_splits(i, o, B, base) for i, o in zip(self.in_ld, self.spec.hidden)]

    def all_groups(self):
        """Every ParamGroup: the branches', then batch norm's of each hidden layer."""
        return [*self.groups.values(), *self.bn_groups]

    def dense_params(self):
        """The dense parameters (hidden layers, head or wdl weights + bias, the branches' and batch
        norm's vectors) in the reference layout (numpy); the wide records are caught up first."""
        ww, wz, wn = self._wide_state()
        P = self._export_dense(self.W, self.w_head, ww, self.wb if self.wdl else None, "w")
        if self.ftrl:
            P.update(self._ftrl_export(wz, wn))
        for l, r in enumerate(self.bn_run if self.bn else ()):
            r = r.cpu().numpy()
            P[BN_KEY % (l + 1, "running_mean")], P[BN_KEY % (l + 1, "running_var")] = r[0].copy(), r[1].copy()
        return P

    def dense_state(self):
        """Adam moments of the dense parameters (hidden layers, head / wdl weights, the branches' and
        batch norm's vectors; the running statistics are state, not trained) in the reference layout:
        {"m": {key: array}, "v": {key: array}} (tests; the table's are in adam_state())."""
        _, wm, wv = self._wide_state()
        wbm, wbv = (self.wbm, self.wbv) if self.wdl else (None, None)
        # FTRL: no Adam moments of wdl_weights, its z and n under their own names
        d = {"m": self._export_dense(self.Wm, self.hm, None if self.ftrl else wm, wbm, "m"),
             "v": self._export_dense(self.Wv, self.hv, None if self.ftrl else wv, wbv, "v")}
        if self.ftrl:
            d.update(self._ftrl_export(wm, wv))
        return d

    # ------------------------------------------------------------------ wide records (wdl)
    FTRL_KEYS = ("ftrl/z", "ftrl/n")   # FTRL's linear and accumulator state of wdl_weights, [N + H, 1]
    FTRL_N0 = 0.1                      # initial_accumulator_value

    def _ftrl_reset(self):
        """FTRL's initial state in the planes: z = 0, n = 0.1 (nothing for Adam)."""
        if self.ftrl:
            self.wm.zero_()
            self.wv.zero_()
            self.wv[: self.w_rows].fill_(self.FTRL_N0)

    def _ftrl_export(self, wz, wn):
        return {"ftrl/z": wz[: self.w_rows].cpu().numpy()[:, None].copy(),
                "ftrl/n": wn[: self.w_rows].cpu().numpy()[:, None].copy()}

    def _ftrl_check(self, d, what):
        """Whether d carries FTRL's state; a state of the other wide optimizer is refused."""
        has = [k in d for k in self.FTRL_KEYS]
        if any(has) and not self.ftrl:
            raise ValueError("%s holds FTRL state (%s) of wdl_weights, but this engine has wide_optimizer='adam'"
                             % (what, ", ".join(self.FTRL_KEYS)))
        if self.ftrl and any(has) and not all(has):
            raise ValueError("%s: wide_optimizer='ftrl' needs both %s" % (what, " and ".join(self.FTRL_KEYS)))
        return all(has)

    def _load_ftrl(self, P, what="load_params"):
        """FTRL's z and n from P into the planes (absent: the initial state)."""
        if not self._ftrl_check(P, what) or not self.ftrl:
            self._ftrl_reset()
            return
        for k, t in zip(self.FTRL_KEYS, (self.wm, self.wv)):
            a = np.ascontiguousarray(P[k], np.float32).reshape(-1)
            if a.size != self.w_rows:
                raise ValueError("%s holds %d values for %d wdl_weights rows" % (k, a.size, self.w_rows))
            t.zero_()
            t[: self.w_rows].copy_(torch.from_numpy(a))

    def wide_nonzero(self):
        """Rows of wdl_weights with w != 0 (FTRL's L1 leaves the others at exactly zero)."""
        if not self.wdl:
            raise ValueError("wide_nonzero: only wdl has wide weights")
        w = self._wide_state()[0]
        return int((w[: self.w_rows] != 0).sum().item())

    def _wide_pack(self):
        """Dense wdl_weights (+ moments) -> records {w, m, v, stamp = current step}; FTRL:
        {w, z, n, 0}."""
        n = self.ww.shape[0]
        self.wrec.zero_()
        self.wrec[:n, 0].copy_(self.ww)
        self.wrec[:n, 1].copy_(self.wm)
        self.wrec[:n, 2].copy_(self.wv)
        if self.ftrl:
            return
        self.wrec.view(torch.int32)[:, 3] = int(self.opt[7].item())
        self._wsq_step = -1

    def _wide_state(self):
        """(w, m, v) of wdl_weights as device tensors (records: caught up first), or Nones."""
        if not self.wdl:
            return None, None, None
        if not self.wide_lazy:
            return self.ww, self.wm, self.wv
        if self.wide_flushes:
            self._wide_flush()
        return self.wrec[:, 0], self.wrec[:, 1], self.wrec[:, 2]

    def _wide_flush(self):
        """Every wide record caught up to the current step; the L2 term of the rows the last
        step did not touch (their pre-update w^2) is left in wsq for loss()."""
        if self._wsq_step == self.steps:
            return
        self.wsq.zero_()
        call("dl_wide_rec_flush", ptr(self.wrec), self.w_rows, self.spec.l2, ptr(self.hist), self.hist_len,
             ptr(self.opt), ptr(self.wsq), ptr(self.wacc), _lib.stream_handle())
        self._wsq_step = self.steps

    def _export_dense(self, Ws, head, ww, wb, which):
        """Augmented hidden-layer matrices (bias row, x0 column order), the permuted head vector, the
        wdl weights and the groups' vectors `which` (w, m or v) -> reference keys and layouts."""
        sp = self.spec
        P = {}
        for g in self.all_groups():
            P.update(g.export(which))
        dims = [self.D0] + sp.hidden
        for l in range(len(sp.hidden)):
            Wi = Ws[l].cpu().numpy()
            W = Wi[: dims[l], : dims[l + 1]]
            if l == 0:
                Wr = np.zeros_like(W)
                Wr[sp.x0_ref_rows()] = W
                W = Wr
            P["deep_%d" % l] = W.copy()
            P["deep_bias_%d" % l] = Wi[dims[l], : dims[l + 1]][None, :].copy()
        if self.wdl:
            if ww is not None:
                P["wdl_weights"] = ww[: self.w_rows].cpu().numpy()[:, None].copy()
            P["wdl_bias"] = wb[:1].cpu().numpy().copy()
            return P
        wi = head[: self.head_n].cpu().numpy()
        w = np.empty_like(wi)
        w[sp.head_ref_index()] = wi
        if sp.fm:
            P["deep_fm_weight"], P["deep_fm_bias"] = w[:-1, None].copy(), w[-1:].copy()
        else:
            P["deep_res"], P["deep_res_bias"] = w[:-1, None].copy(), w[-1:].reshape(1, 1).copy()
        return P

    # ------------------------------------------------------------------ row records
    def _pack(self, table, first):
        """Dense table (+ first-order) -> row records with zero Adam moments, stamped
        with the current step (a fully caught-up state)."""
        E = self.spec.E
        n = table.shape[0]
        self.rec.zero_()
        self.rec[:n, :E].copy_(table)
        if first is not None:
            self.rec[: first.shape[0], E].copy_(first)
        self.rec.view(torch.int32)[:, E + 3] = int(self.opt[7].item())
        self.since_flush = 0
        self.planes_step = -1   # the planes (if any) no longer match the records
        torch.cuda.synchronize()

    def flush(self, planes=False):
        """Catch every row record up to the current step (no-op for the dense engine).
        planes=True also writes every row's p and first-order weight out as dense planes
        (the table predict's plain lookup reads, _forward)."""
        if not self.lazy:
            return
        pp = w1 = None
        flags = self.rec_flags
        if planes and self.p_plane is None:
            # FM models: one slot plane, rows x 2E f32 (p, then the first-order weight in column E:
            # an FM reference's row and weight in one 128-B slot, one random request instead of
            # two — 3.3 GB at 26 M rows, E = 16); otherwise a rows x E p plane (1.7 GB).  Dropped
            # again when training resumes (train_step); without the memory, predict reads the
            # records instead
            try:
                self.p_plane = torch.empty(self.rec.shape[0], 2 * self.spec.E if self.spec.fm else self.spec.E,
                                           device=self.dev)
                self.w1_plane = None
            except torch.cuda.OutOfMemoryError:
                self.p_plane = self.w1_plane = None
                self.flat_planes = False
                planes = False
        if planes:
            pp, w1 = self.p_plane, self.w1_plane
            if self.spec.fm:
                flags |= _lib.REC_PLANE_SLOTS
        self._c("rec_flush", "dl_rec_flush", ptr(self.rec), self.rec_ld, self.spec.E, flags,
                self.rec.shape[0], ptr(self.hist), self.hist_len, ptr(self.opt), ptr(pp), ptr(w1),
                _lib.stream_handle())
        if planes:
            self.planes_step = self.steps
        if self.wide_flushes:
            self._wide_flush()
        self.since_flush = 0

    def plane_lookup(self, B, x0, s, deep=True, gtab=None):
        """The lookup over flush(planes=True)'s planes: FM models read the slot plane (row and
        first-order weight in one 128-B slot, dl_embed_fwd_slots), the others the p plane.
        deep=False: the deep embeddings are not written to x0 (x0_cat_col = -1): the first tower
        layer reads them from the plane itself (fused_gather_l0).  gtab: the deep rows' plane
        offsets go to gtab as well (dl_embed_fwd_gtab, fused_gather_tab) and fm_sum (backward
        only) is not written."""
        L = self._flat_layout(B)
        if not deep:
            L.x0_cat_col = -1
        if gtab is not None:
            self._c("embed_fwd", "dl_embed_fwd_gtab", C_ref(L), ptr(self.p_plane), 1 if self.spec.fm else 0,
                    ptr(self.in_cate), ptr(self.in_cont), ptr(self.in_vec), ptr(x0), ptr(self.fm_out), None,
                    ptr(gtab), ptr(self.err), s)
        elif self.spec.fm:
            self._c("embed_fwd", "dl_embed_fwd_slots", C_ref(L), ptr(self.p_plane),
                    ptr(self.in_cate), ptr(self.in_cont), ptr(self.in_vec), ptr(x0), ptr(self.fm_out),
                    ptr(self.fm_sum), ptr(self.err), s)
        else:
            self._c("embed_fwd", "dl_embed_fwd", C_ref(L), ptr(self.p_plane), None,
                    ptr(self.in_cate), ptr(self.in_cont), ptr(self.in_vec), ptr(x0), ptr(self.fm_out),
                    ptr(self.fm_sum), ptr(self.err), s)

    def fused_gather_rows(self):
        """Whether the lazy single-GPU forward (rec_gather + the indexed lookup) lets the first
        s3 tower layer gather the deep rows from the batch's compact rows itself
        (dl_gemm_s3_nt_gather_rows: the lookup writes the FM side and x0's cont / pooled columns,
        the layer reads rows_u through the inverse map and writes x0's deep columns for dw_l0 —
        bit-identical to the lookup writing them, tests/test_gpu_parity.py).  Same requirements
        as fused_gather_l0; DLAMD_FUSED_GATHER=0 turns both off."""
        sp = self.spec
        if (os.environ.get("DLAMD_FUSED_GATHER", "1") == "0" or not self.s3 or self.bf or not self.lazy
                or type(self) is not CTREngine):
            return False
        if self.drop:   # the plain first layer reads the dropped x0 (and has the dropout epilogue)
            return False
        if self.bi:     # dl_bi_fwd reads x0's field columns before the first layer runs: the lookup writes them
            return False
        return (self.cat_col == 0 and sp.E in (8, 16, 32, 64) and 0 < sp.S <= 40 and (sp.S * sp.E) % 32 == 0
                and sp.S * sp.E <= self.in_ld[0] and self.rows_u.numel() * 4 < 0xFFFFFF00
                and self.idx_inv is not None)

    def fused_gather_tab(self, B, force=False):
        """Whether predict's fused front takes the table form: the FM-side lookup writes the deep
        rows' plane offsets (dl_embed_fwd_gtab, which reads the same ids) and the first layer
        stages them as they stand instead of loading and range-checking the ids itself
        (dl_gemm_s3_nt_gather_tab) — bit-identical (tests/test_gpu_parity.py).  On top of
        fused_gather_l0: E = 8 / 16 with the FM slots in the lookup's short forms.  Off by
        default (DLAMD_GATHER_TAB=1 turns it on; force: the bench's A/B): measured alone the layer
        runs 7-17 us faster, but the lookup + layer pair moves 0-1 us (profiles/r06y/)."""
        sp = self.spec
        if (os.environ.get("DLAMD_GATHER_TAB", "0") != "1" and not force) or sp.M:
            return False
        if _lib.lib().dl_embed_fwd_gtab_ok(C_ref(self._flat_layout(B))) != 1:
            return False
        n = -(-B // 256) * sp.S * 272
        if self.gtab is None or self.gtab.numel() < n:
            self.gtab = torch.empty(n, dtype=torch.int32, device=self.dev)
        return True

    def fused_gather_l0(self):
        """Whether predict on current planes fuses the deep lookup into the first tower layer
        (dl_gemm_s3_nt_gather: the f32 tower's A stream reads each sample's embedding rows from
        the plane through its ids, x0's deep columns are never written or read — bit-identical
        to the lookup + GEMM pair, tests/test_gpu_parity.py).  The s3 tower only, the deep
        columns first in x0 and whole 32-deep chunks, a plane within one 32-bit buffer range;
        DLAMD_FUSED_GATHER=0 turns it off."""
        sp = self.spec
        if os.environ.get("DLAMD_FUSED_GATHER", "1") == "0" or not self.s3 or self.bf or sp.M:
            return False
        if self.reads_x0:   # the fused forms leave x0's deep columns unwritten
            return False
        if self.bn:   # the fused forms apply the ReLU themselves; layer 0 must store its pre-activation
            return False
        pl = self.p_plane
        return (pl is not None and self.cat_col == 0 and sp.E in (8, 16, 32, 64) and 0 < sp.S <= 40
                and (sp.S * sp.E) % 32 == 0 and sp.S * sp.E <= self.in_ld[0]
                and pl.shape[0] * pl.shape[1] * 4 < 0xFFFFFF00)

    def adam_state(self):
        """Table Adam state in the dense layout (tests, checkpoints): dict of m, v (+ m1, v1) as
        numpy.  The device keeps the root state s = sqrt(v) (csrc/common.h adam_elem_root);
        v is exported as fl(s * s).  With wide_optimizer="ftrl" the wide weights' z and n come
        along as "ftrl/z", "ftrl/n"."""
        E, N = self.spec.E, self.N
        ftrl = self._ftrl_export(*self._wide_state()[1:]) if self.ftrl else {}
        if not self.lazy:
            d = {"m": self.tm[:N].cpu().numpy(), "v": _root_to_v(self.tv[:N])}
            if self.first is not None:
                d["m1"], d["v1"] = self.fmm[:N].cpu().numpy(), _root_to_v(self.fmv[:N])
            return dict(d, **ftrl)
        self.flush()
        r = self.rec[:N]
        d = {"m": r[:, E + 4: 2 * E + 4].cpu().numpy(), "v": _root_to_v(r[:, 2 * E + 4: 3 * E + 4])}
        if self.spec.fm:
            d["m1"], d["v1"] = r[:, E + 1].cpu().numpy(), _root_to_v(r[:, E + 2])
        return dict(d, **ftrl)

    def set_adam_state(self, d):
        """Inverse of adam_state() (v imported as s = fl(sqrt(v))); for records, stamps the rows
        with the current step.  A state of the other wide optimizer (FTRL's z / n into an Adam
        engine, or none of them into an FTRL engine) is refused."""
        E, N = self.spec.E, self.N
        if not self._ftrl_check(d, "set_adam_state") and self.ftrl:
            raise ValueError("set_adam_state: an Adam-mode state (no %s) cannot restore an engine with "
                             "wide_optimizer='ftrl'" % ", ".join(self.FTRL_KEYS))
        if self.ftrl:
            self._load_ftrl(d, "set_adam_state")
            if self.wide_lazy:
                n = self.ww.shape[0]
                self.wrec[:n, 1].copy_(self.wm)
                self.wrec[:n, 2].copy_(self.wv)
        t = lambda k: torch.from_numpy(np.ascontiguousarray(d[k], np.float32)).to(self.dev)
        s = lambda k: torch.from_numpy(_v_to_root(d[k])).to(self.dev)
        if not self.lazy:
            self.tm[:N].copy_(t("m"))
            self.tv[:N].copy_(s("v"))
            if self.first is not None and "m1" in d:
                self.fmm[:N].copy_(t("m1"))
                self.fmv[:N].copy_(s("v1"))
            return
        self.rec[:N, E + 4: 2 * E + 4].copy_(t("m"))
        self.rec[:N, 2 * E + 4: 3 * E + 4].copy_(s("v"))
        if self.spec.fm and "m1" in d:
            self.rec[:N, E + 1].copy_(t("m1"))
            self.rec[:N, E + 2].copy_(s("v1"))
        self.rec.view(torch.int32)[:, E + 3] = int(self.opt[7].item())
        self.since_flush = 0
        self.planes_step = -1

    # ------------------------------------------------------------------ inputs
    def stage(self, batch):
        """Copy one batch (dict of tensors/arrays, reference keys) into the static slots."""
        sp = self.spec
        lab = batch["label"]
        B = int(np.prod(lab.shape))
        if B > self.B:
            raise ValueError("batch %d > engine max_batch %d" % (B, self.B))
        _copy_in(self.in_label[:B], lab, F32, self.dev)
        if sp.C:
            _copy_in(self.in_cont[:B, : sp.C], batch["cont_feats"], F32, self.dev)
        if sp.V:
            _copy_in(self.in_vec[:B, : sp.V], batch["vector_feats"], F32, self.dev)
        _copy_in(self.in_cate[:B, : sp.cate_ld], batch["cate_feats"], torch.int64, self.dev)
        if sp.Fw:
            _copy_in(self.in_wide[:B, : sp.Fw], batch["wide_feats"], torch.int64, self.dev)
        if self.weighted:
            w = batch.get("weight")
            if w is None:
                self.in_weight[:B].fill_(1.0)
            else:
                n = int(np.prod(np.shape(w)))
                if n != B:
                    raise ValueError("batch weight holds %d values for %d labels" % (n, B))
                _copy_in(self.in_weight[:B], w, F32, self.dev)
        return B

    # ------------------------------------------------------------------ step
    def _cont(self):
        return self.in_cont if self.spec.C else None

    def _c(self, label, name, *args):
        """Launch one C-ABI entry point; with profiling on, bracket it with events
        on the launch stream (bench.py's live per-kernel timing)."""
        if self.prof is None:
            return call(name, *args)
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        call(name, *args)
        e1.record()
        self.prof.append((label, e0, e1))

    @staticmethod
    def _keep_thr(keep):
        return min(int(math.floor(keep * 4294967296.0)), 4294967295)

    @staticmethod
    def _keep_inv(keep):
        return float(np.float32(1.0) / np.float32(keep))

    def _fm_bwd(self, train_name):
        """An FM backward entry point and its trailing arguments: the plain one, or its FM-part
        dropout twin with the stored keep bits and the two factors."""
        if self.fmdrop:
            return train_name + "_fmdrop", (C_ref(self.fm_drop_desc),)
        return train_name, ()

    def _drop_args(self, layer):
        """dl_gemm_s3_nt_drop / dl_dropout_apply's (keep_thr, inv, seed, layer, opt) of tensor
        `layer` (include/dlamd.h "Dropout": 0 = the tower input, l + 1 = hidden layer l's output)."""
        keep = self.drop[layer]
        return self._keep_thr(keep), self._keep_inv(keep), self.seed & 0xFFFFFFFFFFFFFFFF, layer, ptr(self.opt)

    def _dropping(self, layer):
        return bool(self.drop) and self.drop[layer] < 1.0

    def _forward(self, B, s, train=False):
        """The forward's launches: the embedding front, the deep tower, the head (and its loss
        gradient dz, dh[-1])."""
        fused = self._embed_front(B, s, train)
        if train and self._dropping(0):
            # input dropout on x0's deep_in columns (the bias "ones" column stays); predict never drops
            self._c("drop_x0", "dl_dropout_apply", ptr(self.x0), B, self.D0, self.in_ld[0], *self._drop_args(0),
                    None, s)
        if self.bi:
            # q into x0's columns after the fields, from the field columns the lookup has written
            self._c("bi_fwd", "dl_bi_fwd", B, self.spec.afm_fields, self.spec.E, ptr(self.x0), self.in_ld[0], self.cat_col,
                    ptr(self.x0), self.in_ld[0], self.bi_col, s)
        self._tower_fwd(B, s, train, fused)
        self._head(B, s, train)

    def _embed_front(self, B, s, train):
        """The embedding lookups into x0 and the FM part (pooled, planes, flushed, lazy or dense
        tables).  Returns how the first tower layer gathers the deep rows itself: False (it
        does not), True / "tab" (predict on planes) or "rows" (lazy training)."""
        sp = self.spec
        L = self.layout
        L.batch = B
        x0 = self.x0b if self.x0_direct else self.x0
        fused = False   # the deep lookup inside the first tower layer
        if sp.M and not self.lazy:  # pooled vectors must be in x0 before the FM second order reads them
            self._c("pool_fwd", "dl_pool_fwd", C_ref(L), ptr(self.table), ptr(self.first) if sp.fm else None,
                 ptr(self.in_cate), sp.S, ptr(self.slot_start), ptr(self.slot_end), sp.M, self.fm_pool_col,
                 ptr(self.x0), ptr(self.fm_out), ptr(self.cnt_emb), ptr(self.cnt_first), ptr(self.err), s)
        if (not train and self.lazy and not sp.M and self.since_flush == 0 and type(self) is CTREngine
                and self.planes_step == self.steps):
            # predict on a flushed table whose planes are current (flush(planes=True) at this
            # step): the plain lookup of the dense layout (dl_embed_fwd_slots / dl_embed_fwd),
            # its deep rows read by the first tower layer itself where it can (fused_gather_l0)
            fused = self.fused_gather_l0()
            if fused and self.fused_gather_tab(B):
                fused = "tab"
            self.plane_lookup(B, x0, s, deep=not fused, gtab=self.gtab if fused == "tab" else None)
        elif (not train and self.lazy and not sp.M and self.since_flush == 0 and type(self) is CTREngine
              and sp.F <= sp.REC_FWD_MAX_FM):
            # predict on a flushed table (every record caught up to the current step): the plain
            # lookup, each reference reading its record's first line (dl_embed_fwd_rec_flat; it
            # takes at most 64 FM fields: wider models go through the gather + indexed lookup below)
            if self.n_rep:   # the replicated FM cont-field rows, compact
                self._c("rec_gather", "dl_rec_gather", C_ref(L), ptr(self.rec), self.rec_ld, self.rec_flags, self.n_rep,
                        ptr(self.idx_uniq), None, 0, 1, ptr(self.hist), self.hist_len, ptr(self.opt), 0,
                        ptr(self.rows_u), ptr(self.rows_u1), None, s)
            self._c("embed_fwd", "dl_embed_fwd_rec_flat", C_ref(L), ptr(self.rec), self.rec_ld, self.rec_flags,
                    ptr(self.rows_u), ptr(self.rows_u1) if sp.fm else None, ptr(self.in_cate), ptr(self.in_cont),
                    ptr(self.in_vec), ptr(self.opt), ptr(x0), ptr(self.fm_out), ptr(self.fm_sum), ptr(self.err), s)
        elif self.lazy:
            # rows of the batch (index built by _pre), caught up to the step being taken
            self._c("rec_gather", "dl_rec_gather", C_ref(L), ptr(self.rec), self.rec_ld, self.rec_flags, self.n_rep,
                    ptr(self.idx_uniq), ptr(self.idx_n), B * self.n_slot, 1, ptr(self.hist), self.hist_len,
                    ptr(self.opt), 1 if train else 0, ptr(self.rows_u), ptr(self.rows_u1),
                    ptr(self.mv_u) if (train and self.mv_u is not None) else None, s)
            if sp.M:
                self._c("pool_fwd", "dl_pool_fwd_indexed", C_ref(L), ptr(self.rows_u),
                        ptr(self.rows_u1) if sp.fm else None, ptr(self.idx_inv), self.n_rep, ptr(self.slot_start),
                        ptr(self.slot_end), sp.M, self.fm_pool_col, ptr(self.x0), ptr(self.fm_out), ptr(self.cnt_emb),
                        ptr(self.cnt_first), s)
            # the deep rows go to x0 through the first tower layer where it can gather them
            # (fused_gather_rows: dl_gemm_s3_nt_gather_rows writes x0's deep columns itself)
            fused = "rows" if self.fused_gather_rows() else False
            Lx = L
            if fused:
                Lx = type(L).from_buffer_copy(L)
                Lx.x0_cat_col = -1
            self._c("embed_fwd", "dl_embed_fwd_indexed", C_ref(Lx), ptr(self.rows_u),
                    ptr(self.rows_u1) if sp.fm else None, ptr(self.idx_inv), self.n_rep, ptr(self.in_cont),
                    ptr(self.in_vec), ptr(x0), ptr(self.fm_out), ptr(self.fm_sum), s)
        else:
            self._c("embed_fwd", "dl_embed_fwd", C_ref(L), ptr(self.table), ptr(self.first), ptr(self.in_cate),
                    ptr(self.in_cont), ptr(self.in_vec), ptr(x0), ptr(self.fm_out), ptr(self.fm_sum),
                    ptr(self.err), s)
        return fused

    def _tower_fwd(self, B, s, train=False, fused=False):
        """The deep tower's forward from x0 (f32 / three-plane split on bf16 MFMA / bf16 tower),
        shared with ShardedCTREngine.  fused: the first layer gathers the deep rows itself
        (_embed_front); train: the dropout epilogue where a layer's output drops."""
        sp = self.spec
        nl = len(sp.hidden)
        if self.bf:
            # bf16 tower: x0 -> bf16, ReLU layers on bf16 MFMA (fp32 accumulate), the last layer's
            # output kept fp32 for the fp32 head / wide cross logit (config C5)
            if not self.x0_direct:
                self._c("cast_x0", "dl_cast_bf16", ptr(self.x0), B, self.in_ld[0], self.in_ld[0], ptr(self.x0b),
                        self.in_ld[0], s)
            xb = self.x0b
            for l, hdim in enumerate(sp.hidden):
                last = l == nl - 1
                out = self.h[l] if last else self.hb[l]
                self._c("gemm_fwd_l%d" % l, "dl_gemm_bf16", 0, 1, B, hdim, self.in_ld[l], ptr(xb), self.in_ld[l],
                        ptr(self.WbT[l]), self.in_ld[l], ptr(out), self.h_ld[l], 0 if last else 1, 1, None, 0, 1,
                        0, s)
                if not last:
                    xb = self.hb[l]
        elif self.s3:
            x = self.x0
            for l, hdim in enumerate(sp.hidden):
                bits = (ptr(self.hbits[l]), self.hbits_ld[l]) if l < len(self.hbits) else (None, 0)
                # product layer: layer 0 stores its pre-activation; dl_pnn_inner_fwd adds lp and applies
                # the ReLU (and writes the sign bitmask) in place
                epi = 0 if l == 0 and self.pnn else 1
                if l == 0 and self.pnn:
                    pnn_bits, bits = bits, (None, 0)
                # batch normalisation: every layer stores its pre-activation; _bn_fwd normalises it and
                # applies the ReLU (and writes the sign bitmask) in place
                if self.bn:
                    epi, bn_bits, bits = 0, bits, (None, 0)
                if l == 0 and fused == "rows":
                    # the training form: rows_u through the inverse map (deep slots after the FM
                    # slots), x0's deep columns written for the weight gradient
                    off = sp.S if sp.fm else 0
                    self._c("gemm_fwd_l0", "dl_gemm_s3_nt_gather_rows", B, hdim, self.in_ld[0], ptr(x), self.in_ld[0],
                            ptr(self.rows_u), self.rows_u.shape[0], sp.E, ptr(self.idx_inv[off:]), self.n_slot,
                            self.n_rep, sp.S, sp.E, ptr(self.WTp[0]), self.in_ld[0], self.in_ld[0] * self.out_ld[0],
                            ptr(self.h[0]), self.h_ld[0], epi, *bits, s)
                elif l == 0 and fused == "tab":
                    # predict's table form: the rows' offsets staged from gtab
                    FL = self._flat_layout(B)
                    self._c("gemm_fwd_l0", "dl_gemm_s3_nt_gather_tab", B, hdim, self.in_ld[0], ptr(x), self.in_ld[0],
                            ptr(self.p_plane), FL.n_rows, self.p_plane.shape[1], ptr(self.gtab), sp.S, sp.E,
                            ptr(self.WTp[0]), self.in_ld[0], self.in_ld[0] * self.out_ld[0], ptr(self.h[0]),
                            self.h_ld[0], 1, *bits, s)
                elif l == 0 and fused:
                    FL = self._flat_layout(B)
                    self._c("gemm_fwd_l0", "dl_gemm_s3_nt_gather", B, hdim, self.in_ld[0], ptr(x), self.in_ld[0],
                            ptr(self.p_plane), FL.n_rows, self.p_plane.shape[1], ptr(self.in_cate), FL.cate_ld,
                            FL.deep_cate_offset, FL.zero_row0, sp.S, sp.E, ptr(self.WTp[0]), self.in_ld[0],
                            self.in_ld[0] * self.out_ld[0], ptr(self.h[0]), self.h_ld[0], 1, *bits, s)
                elif train and self._dropping(l + 1):
                    # ReLU + dropout in the epilogue; the bitmask holds (h > 0) & keep
                    self._c("gemm_fwd_l%d" % l, "dl_gemm_s3_nt_drop", B, hdim, self.in_ld[l], ptr(x), self.in_ld[l],
                            ptr(self.WTp[l]), self.in_ld[l], self.in_ld[l] * self.out_ld[l], ptr(self.h[l]),
                            self.h_ld[l], 1, None, 0, *bits, *self._drop_args(l + 1), s)
                else:
                    self._c("gemm_fwd_l%d" % l, "dl_gemm_s3_nt_bits", B, hdim, self.in_ld[l], ptr(x), self.in_ld[l],
                            ptr(self.WTp[l]), self.in_ld[l], self.in_ld[l] * self.out_ld[l], ptr(self.h[l]),
                            self.h_ld[l], epi, None, 0, *bits, s)
                if l == 0 and self.pnn:
                    self._pnn_fwd(B, pnn_bits, s)
                if self.bn:
                    self._bn_fwd(l, B, bn_bits, train, s)
                x = self.h[l]
        else:
            x = self.x0
            for l, hdim in enumerate(sp.hidden):
                self._c("gemm_fwd_l%d" % l, "dl_gemm_f32", 0, 0, B, hdim, self.in_ld[l], ptr(x), self.in_ld[l],
                        ptr(self.W[l]), self.out_ld[l], ptr(self.h[l]), self.h_ld[l],
                        0 if (l == 0 and self.pnn) or self.bn else 1, None, 0, 1, 0, s)
                if l == 0 and self.pnn:   # (the f32 path reads the ReLU's sign from h[0] itself)
                    self._pnn_fwd(B, (None, 0), s)
                if self.bn:
                    self._bn_fwd(l, B, (None, 0), train, s)
                x = self.h[l]

    def _bn_fwd(self, l, B, bits, train, s):
        """h[l] = relu(gamma xhat + beta) on layer l's stored pre-activation: a training step takes the
        batch's statistics (kept in bn_stat[l], xhat in hx[l], for the backward) and updates the running
        ones under the step guard; predict normalises by the running ones."""
        sp = self.spec
        D, run = sp.hidden[l], self.bn_run[l]
        if train:
            self._c("bn_stats_l%d" % l, "dl_bn_stats", B, D, ptr(self.h[l]), self.h_ld[l], sp.bn_eps, sp.bn_momentum,
                    ptr(self.bn_stat[l]), ptr(run[0]), ptr(run[1]), ptr(self.opt), ptr(self.bn_ws),
                    self.bn_ws.numel(), s)
            self._c("bn_fwd_l%d" % l, "dl_bn_fwd", B, D, ptr(self.h[l]), self.h_ld[l], ptr(self.bn_stat[l]), None,
                    None, sp.bn_eps, ptr(self.bn_groups[l].w), ptr(self.hx[l]), self.h_ld[l], *bits, s)
        else:
            self._c("bn_fwd_l%d" % l, "dl_bn_fwd", B, D, ptr(self.h[l]), self.h_ld[l], None, ptr(run[0]),
                    ptr(run[1]), sp.bn_eps, ptr(self.bn_groups[l].w), None, 0, *bits, s)

    def _bn_bwd(self, l, B, s):
        """Layer l's batch-norm backward on the ReluGrad-masked dh[l]: dgamma / dbeta as slab rows for
        the layer's Adam, then dh[l] rewritten in place into the gradient of the pre-activation."""
        D, g = self.spec.hidden[l], self.bn_groups[l]
        nb = g.rows(B)
        self._c("bn_sums_l%d" % l, "dl_bn_bwd_sums", B, D, ptr(self.dh[l]), self.h_ld[l], ptr(self.hx[l]),
                self.h_ld[l], ptr(g.slab), nb, s)
        self._c("bn_apply_l%d" % l, "dl_bn_bwd_apply", B, D, ptr(self.dh[l]), self.h_ld[l], ptr(self.hx[l]),
                self.h_ld[l], ptr(g.w), ptr(self.bn_stat[l]), ptr(g.slab), nb, ptr(self.bn_sums), s)

    def _pnn_fwd(self, B, bits, s):
        """h[0] = relu(h[0] + lp): the product layer on layer 0's stored pre-activation (x0 is complete:
        in lazy training the first layer's fused row gather wrote its deep columns)."""
        sp = self.spec
        self._c("pnn_fwd", "dl_pnn_inner_fwd", B, sp.afm_fields, sp.E, sp.hidden[0], ptr(self.x0), self.in_ld[0],
                self.cat_col, ptr(self.groups["pnn"].w), ptr(self.h[0]), self.h_ld[0], *bits, s)

    def _head(self, B, s, train):
        """The output layer, the loss and its gradients dz and dh[-1]: the wdl cross logit (wide
        rows dense or lazy), or the FM / deep_res head (plain, FM-part dropout, cross network)."""
        sp = self.spec
        H = sp.hidden[-1]
        # the loss scale: the host constant 1 / B, or in a weighted training step the *_weighted
        # twins' (w_eff, norm) — predict ignores the weights
        sw, scale = ("_weighted", (ptr(self.w_eff), ptr(self.norm))) if train and self.weighted else ("", (1.0 / B,))
        if self.wdl and self.wide_lazy:
            # the batch's wide rows caught up into the compact local table, the head on local ids
            fn, dh_last = ("dl_wdl_head_fwd_bwd_bf16", self.dhb[-1]) if self.bf else ("dl_wdl_head_fwd_bwd", self.dh[-1])
            nw = B * sp.Fw
            if self.ftrl:   # the records as they stand: FTRL rows never lag
                self._c("wide_gather", "dl_wide_ftrl_gather", ptr(self.wrec), self.w_rows, ptr(self.widx_uniq),
                        ptr(self.widx_n), nw, sp.Fw, H, ptr(self.opt), ptr(self.wloc),
                        ptr(self.wstash) if train else None, s)
            else:
                self._c("wide_gather", "dl_wide_rec_gather", ptr(self.wrec), self.w_rows, ptr(self.widx_uniq),
                        ptr(self.widx_n), nw, sp.Fw, H, ptr(self.hist), self.hist_len, ptr(self.opt), sp.l2,
                        1 if train else 0, ptr(self.wloc), ptr(self.wstash) if train else None,
                        ptr(self.wrep) if train else None, s)
            self._c("head", fn + sw, B, sp.Fw, H, ptr(self.in_wide_loc), sp.Fw, ptr(self.h[-1]), self.h_ld[-1],
                    ptr(self.wloc), ptr(self.wb), sp.Fw + H + nw, ptr(self.in_label), sp.logloss_eps, *scale,
                    ptr(self.score), ptr(self.z), ptr(self.dz), ptr(dh_last), None, None,
                    ptr(self.head_slab), self.head_blocks, ptr(self.err), s)
            if train:   # the wide rows' gradient: segment sums over the wide index (no atomics)
                self._c("wide_grad", "dl_wide_seg_grad", ptr(self.dz), sp.Fw, ptr(self.widx_refs), ptr(self.widx_off),
                        ptr(self.widx_n), nw, nw, ptr(self.wgloc[sp.Fw + H:]), ptr(self.wlong), ptr(self.opt), s)
            return
        if self.wdl:
            # bf16 tower: dY of the last layer written as bf16 by the head itself (no cast pass)
            fn, dh_last = ("dl_wdl_head_fwd_bwd_bf16", self.dhb[-1]) if self.bf else ("dl_wdl_head_fwd_bwd", self.dh[-1])
            self._c("head", fn + sw, B, sp.Fw, H, ptr(self.in_wide), self.in_wide.shape[1],
                    ptr(self.h[-1]), self.h_ld[-1], ptr(self.ww), ptr(self.wb), self.w_rows, ptr(self.in_label),
                    sp.logloss_eps, *scale, ptr(self.score), ptr(self.z), ptr(self.dz), ptr(dh_last),
                    ptr(self.wg) if train else None, ptr(self.w_touched) if train else None,
                    ptr(self.head_slab), self.head_blocks, ptr(self.err), s)
            return
        if train and self.fmdrop:   # predict / evaluate never drop
            k1, k2 = self.fmdrop
            self._c("head", "dl_head_fwd_bwd_fmdrop" + sw, B, sp.fm_cols, H, ptr(self.fm_out), self.fm_ld,
                    ptr(self.h[-1]), self.h_ld[-1], ptr(self.w_head), ptr(self.in_label), sp.logloss_eps, *scale,
                    ptr(self.score), ptr(self.z), ptr(self.dz), ptr(self.dh[-1]), ptr(self.head_slab),
                    self.head_blocks, sp.F, self._keep_thr(k1), self._keep_inv(k1), self._keep_thr(k2),
                    self._keep_inv(k2), self.seed & 0xFFFFFFFFFFFFFFFF, ptr(self.opt), ptr(self.fm_keep), s)
            return
        if self.chain:
            # x0 is complete here (in lazy training the first layer's fused row gather wrote its deep columns):
            # every member's logit with the one before it added (z_in; NULL for the first), then the head with
            # the last as its extra logit
            z_extra = None
            for c in self.chain:
                x0 = (ptr(self.x0), self.in_ld[0]) if c.whole_x0 else (ptr(self.x0), self.in_ld[0], self.cat_col)
                z_in = () if c.whole_x0 else (ptr(z_extra),)
                self._c(*c.fwd, B, *c.lead, *x0, ptr(c.g.w), *z_in, *map(ptr, c.state), ptr(c.z), s)
                z_extra = c.z
            self._c("head", "dl_head_fwd_bwd_cross" + sw, B, sp.fm_cols, H, ptr(self.fm_out), self.fm_ld,
                    ptr(self.h[-1]), self.h_ld[-1], ptr(self.w_head), ptr(self.in_label), sp.logloss_eps, *scale,
                    ptr(z_extra), ptr(self.score), ptr(self.z), ptr(self.dz),
                    ptr(self.dh[-1]), ptr(self.head_slab), self.head_blocks, s)
            return
        self._c("head", "dl_head_fwd_bwd" + sw, B, sp.fm_cols, H, ptr(self.fm_out), self.fm_ld, ptr(self.h[-1]),
             self.h_ld[-1], ptr(self.w_head), ptr(self.in_label), sp.logloss_eps, *scale,
             ptr(self.score), ptr(self.z), ptr(self.dz), ptr(self.dh[-1]), ptr(self.head_slab),
             self.head_blocks, s)

    def _pre(self, B, weights=True):
        """The batch's validation and index build, before its step begins: the batch's
        validation word is reset, then set by dl_validate_batch for every id no index build
        checks (the dense-layout gathers' cate ids, wdl's wide ids) and by dl_index_build (the
        hand-written radix sort + segmented unique of index.hip, no host synchronisation).
        Runs on the current stream — inside the step's hipGraph (graph=True), or on the side
        stream when prefetched — so a bad batch is known before dl_step_begin opens its step.
        With sample weighting (and `weights`: a training batch) dl_weight_norm follows the
        validation: the effective weights, the loss normaliser and the bad-weight bit."""
        s = _lib.stream_handle()
        L = self.layout
        L.batch = B
        sp = self.spec
        cate = self.in_cate if self.bwd != "sorted" else None
        wide = self.in_wide if self.wdl else None
        self._c("validate", "dl_validate_batch", C_ref(L), ptr(cate), ptr(wide), sp.Fw if wide is not None else 0,
                self.in_wide.shape[1], self.w_rows, 1, ptr(self.err), s)
        if self.weighted and weights:
            self._c("weight_norm", "dl_weight_norm", ptr(self.in_weight), ptr(self.in_label), B, sp.pos_weight,
                    ptr(self.w_eff), ptr(self.norm), ptr(self.err), s)
        if self.bwd != "sorted":
            return
        if self.wide_lazy:
            # the table ids and the wide ids in one build, then the head's local wide ids
            WL = self.wlayout
            WL.batch = B
            self._c("index_build", "dl_index_build_pair", C_ref(L), ptr(self.in_cate), C_ref(WL), ptr(self.in_wide),
                    ptr(self.idx_ws), self.idx_ws.numel(), ptr(self.idx_keys), ptr(self.idx_refs),
                    ptr(self.idx_uniq), ptr(self.idx_off), ptr(self.idx_n), ptr(self.idx_inv), ptr(self.widx_uniq),
                    ptr(self.widx_refs), ptr(self.widx_off), ptr(self.widx_n), ptr(self.winv), ptr(self.err), s)
            call("dl_wide_local_ids", ptr(self.winv), B * sp.Fw, sp.Fw + sp.hidden[-1], ptr(self.in_wide_loc), s)
            return
        # single GPU: keys are the rows themselves (replicated rows need no owner group;
        # the record kernels recognise them by row < n_rep) — the narrowest sort range
        self._c("index_build", "dl_index_build", C_ref(L), ptr(self.in_cate), 1, 0, ptr(self.idx_ws),
                self.idx_ws.numel(), ptr(self.idx_keys), ptr(self.idx_refs), ptr(self.idx_uniq),
                ptr(self.idx_off), ptr(self.idx_n), ptr(self.idx_inv) if self.lazy else None, None,
                ptr(self.err), s)

    def _train(self, B):
        """The step's launches: forward, the tower's backward and dense Adam, the embedding
        backward and the remaining updates (_train_back), the step's loss into the running sum."""
        sp = self.spec
        s = _lib.stream_handle()
        L = self.layout
        # a batch whose ids failed validation (index build) poisons the step: nothing is applied
        # (dl_step_begin: the guard, the Adam step begin and the lazy tables' alpha ring entry)
        self._c("step_begin", "dl_step_begin", ptr(self.err), ptr(self.opt), sp.decay_rate, float(sp.decay_steps),
                ptr(self.hist) if self.lazy else None, self.hist_len if self.lazy else 0, s)
        self._forward(B, s, train=True)
        nl = len(sp.hidden)
        if self._dropping(nl):
            # the head masked dh[-1] by h[-1] > 0, the combined bit of the dropped h[-1]: the
            # 1/keep factor is what is missing (re-applying the regenerated mask changes nothing)
            self._c("drop_dh", "dl_dropout_apply", ptr(self.dh[-1]), B, sp.hidden[-1], self.h_ld[-1],
                    *self._drop_args(nl), None, s)
        dws = self._dw_splits(B, fixed="DLAMD_DW_SPLITS" in os.environ)
        self._cast_dh(B, s)
        fused = self._adam_fused()
        for l in reversed(range(nl)):
            # fused: every layer's weight and input gradients, then one launch for the dense Adams
            # (each layer's W planes are read by its dX first; nothing else reads W before the next
            # step); else each layer's Adam after its input gradient
            if self.bn:   # dh[l] becomes the pre-activation's gradient before the layer's GEMMs read it
                self._bn_bwd(l, B, s)
            self._tower_dw(l, B, dws[l], self.w_slabs[l], s)
            if self.bn:
                # the layer's own bias: its exact gradient, 0, in place of the weight gradient's noise row
                self._c("bn_bias_l%d" % l, "dl_bn_zero_bias_grad", ptr(self.w_slabs[l]),
                        _num_splits(B, dws[l], 64 if (self.bf or self.s3) else 16), self.in_ld[l] * self.out_ld[l],
                        ([self.D0] + sp.hidden)[l] * self.out_ld[l], self.out_ld[l], s)
            self._tower_dx(l, B, s)
            if not fused:
                self._tower_adam(l, self.w_slabs[l], _num_splits(B, dws[l], 64 if (self.bf or self.s3) else 16), s)
        if fused:
            lay = (_lib.AdamLayer * nl)()
            for l in range(nl):
                l2, l2n, l1, reg_sum = self._layer_reg(l)
                lay[l] = _lib.AdamLayer(ptr(self.W[l]), ptr(self.Wm[l]), ptr(self.Wv[l]), ptr(self.w_slabs[l]),
                                        self.in_ld[l] * self.out_ld[l], l2n, reg_sum,
                                        ptr(self.Wp[l] if self.s3 else self.Wb[l]),
                                        ptr(self.WTp[l] if self.s3 else self.WbT[l]),
                                        _num_splits(B, dws[l], 64), self.in_ld[l], self.out_ld[l], l1, l2, 0)
            self._adam_lay = lay   # kept alive: a captured graph's kernel arguments were copied at launch
            self._c("adam_dense", "dl_adam_dense_layers", nl, C_ref(lay), 3 if self.s3 else 1, ptr(self.opt), s)
        for c in self.chain:
            # gemm_dx_l0 has written dx0 (the embedding columns of x0, from column cat_col); every chain member's
            # share is added before the embedding backward reads it (the cross network's over its own window)
            x0 = (ptr(self.x0), self.in_ld[0]) if c.whole_x0 else (ptr(self.x0), self.in_ld[0], self.cat_col)
            window = (self.cat_col, self.dx_cols) if c.whole_x0 else (0,)
            self._c(*c.bwd, B, *c.lead, *x0, ptr(c.g.w), *map(ptr, c.state), ptr(self.dz), ptr(self.dx0), self.dx_ld,
                    *window, ptr(c.g.slab), c.g.blocks, s)
        if self.pnn:
            # the product layer's share, from the ReluGrad-masked dh[0] the tower's backward formed
            g = self.groups["pnn"]
            self._c("pnn_bwd", "dl_pnn_inner_bwd", B, sp.afm_fields, sp.E, sp.hidden[0], ptr(self.x0), self.in_ld[0],
                    self.cat_col, ptr(g.w), ptr(self.dh[0]), self.h_ld[0], ptr(self.dx0), self.dx_ld, 0,
                    ptr(g.slab), g.blocks, s)
        if self.bi:
            # the pooling's share: dq is dx0's columns after the fields (gemm_dx_l0's wider range, plus
            # the cross network's share of them), complete here
            self._c("bi_bwd", "dl_bi_bwd", B, sp.afm_fields, sp.E, ptr(self.x0), self.in_ld[0], self.cat_col,
                    ptr(self.dx0), self.dx_ld, self.bi_col, ptr(self.dx0), self.dx_ld, 0, s)
        self._train_back(B, s, L)
        # the step's loss into the running sum (read once per epoch: loss_sum_end)
        width = self.head_slab.shape[1]
        coef = sp.l2 if sp.hidden_reg == "l1" else 0.5 * sp.l2
        if self.weighted:
            self._c("loss_acc", "dl_loss_accumulate_weighted", ptr(self.head_slab), call_int(self.head_grid, B), width,
                    width - 1, ptr(self.norm), ptr(self.opt), coef, ptr(self.loss_acc), ptr(self._ring), s)
            return
        self._c("loss_acc", "dl_loss_accumulate", ptr(self.head_slab), call_int(self.head_grid, B), width, width - 1,
                1.0 / B, ptr(self.opt), coef, ptr(self.loss_acc), ptr(self._ring), s)

    def _cast_dh(self, B, s):
        """The bf16 tower's copy of the head's dh[-1] (the wdl head writes its bf16 dY itself)."""
        if self.bf and not self.wdl:
            self._c("cast_dh", "dl_cast_bf16", ptr(self.dh[-1]), B, self.h_ld[-1], self.h_ld[-1], ptr(self.dhb[-1]),
                    self.h_ld[-1], s)

    # The tower's backward, one layer at a time; ShardedCTREngine launches the same methods (its
    # weight gradients into its one slab, its Adam from the all-reduced flat gradient).
    def _tower_dw(self, l, B, splits, slab, s):
        """The weight gradient of layer l: `splits` split-K slabs over the batch into `slab`."""
        sp = self.spec
        hdim, stride = sp.hidden[l], self.in_ld[l] * self.out_ld[l]
        if self.bf:
            # dW = X^T dY straight from the batch-major bf16 activations and gradients
            # (transposing LDS reads inside the kernel: no X^T / dY^T copies)
            xl = self.x0b if l == 0 else self.hb[l - 1]
            self._c("gemm_dw_l%d" % l, "dl_gemm_bf16", 1, 0, self.in_ld[l], hdim, B, ptr(xl), self.in_ld[l],
                    ptr(self.dhb[l]), self.h_ld[l], ptr(slab), self.out_ld[l], 0, 3, None, 0, splits,
                    stride, s)
        elif self.s3:   # dW = X^T dY (split-K slabs over the batch)
            xin = self.x0 if l == 0 else self.h[l - 1]
            i, o = self.in_ld[l], self.out_ld[l]
            # (a width that is no multiple of 4 is rounded up for the TN kernel: dh's pad columns
            # are zero and stay so, so are their weight gradients)
            self._c("gemm_dw_l%d" % l, "dl_gemm_s3_tn", i, _ru(hdim, 4), B, ptr(xin), i, ptr(self.dh[l]), self.h_ld[l],
                    ptr(slab), o, splits, stride, s)
        else:
            xin = self.x0 if l == 0 else self.h[l - 1]
            self._c("gemm_dw_l%d" % l, "dl_gemm_f32", 1, 0, self.in_ld[l], hdim, B, ptr(xin), self.in_ld[l],
                    ptr(self.dh[l]), self.h_ld[l], ptr(slab), self.out_ld[l], 3, None, 0, splits, stride, s)

    def _tower_dx(self, l, B, s):
        """The input gradient of layer l (ReluGrad by the layer below; l = 0: dx0 in f32)."""
        sp = self.spec
        if self.bf:
            if l > 0:   # dX = dY . W^T, ReluGrad by the bf16 activations, bf16 out
                self._c("gemm_dx_l%d" % l, "dl_gemm_bf16", 0, 1, B, sp.hidden[l - 1], self.out_ld[l],
                        ptr(self.dhb[l]), self.h_ld[l], ptr(self.Wb[l]), self.out_ld[l], ptr(self.dhb[l - 1]),
                        self.h_ld[l - 1], 1, 2, ptr(self.hb[l - 1]), self.h_ld[l - 1], 1, 0, s)
            else:       # dx0 stays fp32 for the embedding backward
                self._c("gemm_dx_l0", "dl_gemm_bf16", 0, 1, B, self.dx_cols, self.out_ld[0], ptr(self.dhb[0]),
                        self.h_ld[0], ptr(self.Wb[0]), self.out_ld[0], ptr(self.dx0), self.dx_ld, 0, 0, None, 0,
                        1, 0, s)
        elif self.s3:   # dX = dY W^T with ReluGrad
            i, o = self.in_ld[l], self.out_ld[l]
            if l > 0 and self._dropping(l):   # ReluGrad and the keep bit from the combined bitmask, times 1/keep
                self._c("gemm_dx_l%d" % l, "dl_gemm_s3_nt_drop", B, sp.hidden[l - 1], o, ptr(self.dh[l]),
                        self.h_ld[l], ptr(self.Wp[l]), o, i * o, ptr(self.dh[l - 1]), self.h_ld[l - 1], 3,
                        None, 0, ptr(self.hbits[l - 1]), self.hbits_ld[l - 1], *self._drop_args(l), s)
            elif l > 0:   # ReluGrad from the forward's sign bitmask
                self._c("gemm_dx_l%d" % l, "dl_gemm_s3_nt_bits", B, sp.hidden[l - 1], o, ptr(self.dh[l]),
                        self.h_ld[l], ptr(self.Wp[l]), o, i * o, ptr(self.dh[l - 1]), self.h_ld[l - 1], 3,
                        None, 0, ptr(self.hbits[l - 1]), self.hbits_ld[l - 1], s)
            else:
                self._c("gemm_dx_l0", "dl_gemm_s3_nt", B, self.dx_cols, o, ptr(self.dh[0]), self.h_ld[0],
                        ptr(self.Wp[0]), o, i * o, ptr(self.dx0), self.dx_ld, 0, None, 0, s)
                if self._dropping(0):   # the input dropout's mask on the embedding columns' gradient
                    self._c("drop_dx0", "dl_dropout_apply", ptr(self.dx0), B, self.dx_cols, self.dx_ld,
                            *self._drop_args(0), None, s)
        else:
            self._c("transpose_l%d" % l, "dl_transpose_f32", ptr(self.W[l]), self.in_ld[l], self.out_ld[l],
                    self.out_ld[l], ptr(self.Wt), self.in_ld[l], s)
            if l > 0:
                self._c("gemm_dx_l%d" % l, "dl_gemm_f32", 0, 0, B, sp.hidden[l - 1], self.out_ld[l],
                        ptr(self.dh[l]), self.h_ld[l], ptr(self.Wt), self.in_ld[l], ptr(self.dh[l - 1]),
                        self.h_ld[l - 1], 2, ptr(self.h[l - 1]), self.h_ld[l - 1], 1, 0, s)
            else:
                self._c("gemm_dx_l0", "dl_gemm_f32", 0, 0, B, self.dx_cols, self.out_ld[0], ptr(self.dh[0]),
                        self.h_ld[0], ptr(self.Wt), self.in_ld[0], ptr(self.dx0), self.dx_ld, 0, None, 0, 1, 0, s)

    def _layer_reg(self, l):
        """(l2, element count, l1 flag, sum-of-squares word) of the regulariser on hidden weight
        matrix l: wdl L2 (wdl.py:272-275), dnn L1 (dnn.py:88-90); the bias row excluded."""
        sp = self.spec
        reg = sp.hidden_reg
        if not reg:
            return 0.0, 0, 0, None
        return sp.l2, ([self.D0] + sp.hidden)[l] * self.out_ld[l], 1 if reg == "l1" else 0, ptr(self.opt[8:])

    def _tower_adam(self, l, grad, nsplit, s):
        """TF1 Adam on layer l from `grad`, `nsplit` slabs one layer's stride apart."""
        stride = self.in_ld[l] * self.out_ld[l]
        l2, l2n, l1, reg_sum = self._layer_reg(l)
        if self.s3 or self.bf:   # the update writes the GEMM operand copies of W and W^T itself
            self._c("adam_dense_l%d" % l, "dl_adam_dense_split3" if self.s3 else "dl_adam_dense_bf16",
                    ptr(self.W[l]), ptr(self.Wm[l]), ptr(self.Wv[l]), ptr(grad), nsplit, stride, self.in_ld[l],
                    self.out_ld[l], l2, l2n, l1, ptr(self.opt), reg_sum,
                    ptr(self.Wp[l] if self.s3 else self.Wb[l]), ptr(self.WTp[l] if self.s3 else self.WbT[l]), s)
            return
        self._c("adam_dense_l%d" % l, "dl_adam_dense_reg", ptr(self.W[l]), ptr(self.Wm[l]), ptr(self.Wv[l]),
                ptr(grad), nsplit, stride, stride, l2, l2n, l1, ptr(self.opt), None, reg_sum, s)
        self._refresh_wb(l, s)   # (launches nothing for an f32 tower)

    def _adam_fused(self):
        """The tower's dense Adams as one launch (dl_adam_dense_layers) after the backward's GEMMs
        (DLAMD_ADAM_FUSED=0: one launch per layer, after its input gradient)."""
        return ((self.s3 or self.bf) and len(self.spec.hidden) <= 4 and type(self) is CTREngine
                and os.environ.get("DLAMD_ADAM_FUSED", "1") != "0")

    def _train_back(self, B, s, L):
        """_train from the embedding backward onwards: the table, head / wide and cross updates."""
        sp = self.spec
        # embedding backward (uses pre-update table and head weights)
        bwd_blocks = call_int("dl_embed_bwd_grid", C_ref(L))
        if self.lazy:
            self._embed_bwd_lazy(B, L, s)
        elif self.bwd == "sorted":
            fn, fd = self._fm_bwd("dl_embed_bwd_sorted")
            self._c("embed_bwd", fn, C_ref(L), ptr(self.table), None, ptr(self.idx_uniq),
                    ptr(self.idx_off), ptr(self.idx_n), ptr(self.idx_refs), 1, B * self.n_slot, ptr(self.dz),
                    ptr(self.w_head), ptr(self.fm_sum), ptr(self.dx0), ptr(self.tg), ptr(self.fmg),
                    ptr(self.touched), 0, None, *fd, s)
            fn, fd = self._fm_bwd("dl_embed_cont_bwd")
            self._c("cont_bwd", fn, C_ref(L), ptr(self.table), ptr(self._cont()), ptr(self.dz),
                    ptr(self.w_head), ptr(self.fm_sum), ptr(self.cont_slab), self.bwd_blocks, *fd, s)
        else:
            fn, fd = self._fm_bwd("dl_embed_bwd")
            self._c("embed_bwd", fn, C_ref(L), ptr(self.table), ptr(self.in_cate), ptr(self._cont()),
                    ptr(self.dz), ptr(self.w_head), ptr(self.fm_sum), ptr(self.dx0), ptr(self.tg), ptr(self.fmg),
                    ptr(self.touched), ptr(self.cont_slab), self.bwd_blocks, *fd, s)
        if not self.lazy:
            self._c("cont_reduce", "dl_embed_cont_reduce", C_ref(L), ptr(self.cont_slab), bwd_blocks, ptr(self.tg),
                    ptr(self.fmg), ptr(self.touched), s)
        if sp.M and not self.lazy:
            fn, fd = self._fm_bwd("dl_pool_bwd")
            self._c("pool_bwd", fn, C_ref(L), ptr(self.in_cate), sp.S, ptr(self.slot_start), ptr(self.slot_end),
                 sp.M, self.fm_pool_col, ptr(self.x0), ptr(self.fm_sum), ptr(self.dz), ptr(self.w_head), ptr(self.dx0),
                 sp.S * sp.E, ptr(self.cnt_emb), ptr(self.cnt_first), ptr(self.tg), ptr(self.fmg),
                 ptr(self.touched), *fd, s)
        H = sp.hidden[-1]
        hb = call_int(self.head_grid, B)
        for g in self.bn_groups:   # (before the families part ways: wdl has gamma and beta too)
            g.adam(self, B, s)
        if self.wdl and self.wide_lazy:
            # wdl_weights, lazy: the deep-output rows' batch sums folded into the local gradient,
            # then TF1 Adam (L2 on every row, wdl.py:270-271) on the batch's unique wide rows and
            # the deep-output rows only; the untouched rows' L2 steps are replayed when read
            self._c("wdl_fold", "dl_slab_fold_rows", ptr(self.head_slab), hb, H + 2, 0, H, ptr(self.wgloc), sp.Fw,
                    None, s)
            self._c("adam_bias", "dl_adam_dense", ptr(self.wb), ptr(self.wbm), ptr(self.wbv),
                    ptr(self.head_slab[:, H:]), hb, H + 2, 1, 0.0, 0, ptr(self.opt), None, None, s)
            if self.ftrl:   # FTRL-proximal on the same rows: nothing joins the step's regulariser sum
                self._c("ftrl_wide", "dl_wide_ftrl_update", ptr(self.wrec), ptr(self.widx_n), B * sp.Fw,
                        ptr(self.wstash), ptr(self.wgloc), sp.Fw, H, sp.ftrl_lr, sp.wide_l1, sp.wide_l2, ptr(self.opt),
                        ptr(self.wdmark), s)
                return
            self._c("adam_wide", "dl_wide_rec_update", ptr(self.wrec), ptr(self.widx_n), B * sp.Fw, ptr(self.wstash),
                    ptr(self.wgloc), sp.Fw, H, sp.l2, ptr(self.hist), self.hist_len, ptr(self.opt), ptr(self.wdmark),
                    ptr(self.wsq_part), ptr(self.wrep), ptr(self.wacc), s)
            return
        if self.wdl:
            # wdl_weights: dense Adam with L2 on every row (wdl.py:270-271); the deep-output
            # rows get their batch sums folded in from the head slab first
            self._c("wdl_fold", "dl_slab_fold_rows", ptr(self.head_slab), hb, H + 2, 0, H, ptr(self.wg), sp.Fw,
                    ptr(self.w_touched), s)
            self._c("adam_bias", "dl_adam_dense", ptr(self.wb), ptr(self.wbm), ptr(self.wbv),
                    ptr(self.head_slab[:, H:]), hb, H + 2, 1, 0.0, 0, ptr(self.opt), None, None, s)
            if self.ftrl:   # FTRL-proximal on the flagged rows of the planes (wm: z, wv: n)
                self._c("ftrl_wide", "dl_ftrl_rows", ptr(self.ww), ptr(self.wm), ptr(self.wv), ptr(self.wg),
                        ptr(self.w_touched), self.ww.shape[0], sp.ftrl_lr, sp.wide_l1, sp.wide_l2, ptr(self.opt), s)
            else:
                self._c("adam_wide", "dl_adam_rows", ptr(self.ww), ptr(self.wm), ptr(self.wv), ptr(self.wg),
                        ptr(self.w_touched), self.ww.shape[0], 1, sp.l2, 1 | _lib.ROWS_GRAD_FIXED, ptr(self.opt),
                        ptr(self.opt[8:]), s)
            if self.lazy:
                return
            self._c("adam_table", "dl_adam_rows", ptr(self.table), ptr(self.tm), ptr(self.tv), ptr(self.tg),
                    ptr(self.touched), self.table.shape[0], sp.E, 0.0, 1 | self.rows_sparse, ptr(self.opt), None, s)
            return
        # head Adam: L2 on the output weights only (deepfm_pipeline.py:183 / dnn_pipeline.py:131)
        self._c("adam_head", "dl_adam_dense", ptr(self.w_head), ptr(self.hm), ptr(self.hv), ptr(self.head_slab),
                hb, sp.fm_cols + H + 2, self.head_n, sp.l2 if sp.head_l2 else 0.0,
                self.head_n - 1 if sp.head_l2 else 0, ptr(self.opt), ptr(self.w_head_prev), ptr(self.opt[8:]), s)
        for g in self.groups.values():   # the branches' vectors, each with its own regulariser arguments
            g.adam(self, B, s)
        if self.lazy:
            return
        if sp.fm:
            self._c("adam_table", "dl_adam_rows", ptr(self.table), ptr(self.tm), ptr(self.tv), ptr(self.tg),
                    ptr(self.touched), self.table.shape[0], sp.E, 0.0, self.rows_sparse, ptr(self.opt), None, s)
            self._c("adam_first", "dl_adam_rows", ptr(self.first), ptr(self.fmm), ptr(self.fmv), ptr(self.fmg),
                    ptr(self.touched), self.first.shape[0], 1, 0.0, 1 | self.rows_sparse, ptr(self.opt), None, s)
        else:
            self._c("adam_table", "dl_adam_rows", ptr(self.table), ptr(self.tm), ptr(self.tv), ptr(self.tg),
                    ptr(self.touched), self.table.shape[0], sp.E, 0.0, 1 | self.rows_sparse, ptr(self.opt), None, s)

    # per-batch buffers: inputs and the batch index.  With prefetching they are double
    # buffered — the next batch is staged and indexed into the other set on a side stream
    # while the current step runs.
    SLOT_ATTRS = ("in_label", "in_cont", "in_vec", "in_cate", "in_wide", "idx_ws", "idx_keys", "idx_refs",
                  "idx_uniq", "idx_off", "idx_n", "idx_inv", "err", "widx_refs", "widx_uniq",
                  "widx_off", "widx_n", "winv", "in_wide_loc", "in_weight", "w_eff", "norm")

    def _side_stream(self):
        if self.side is None:
            # high priority: a hardware queue of its own (a default-priority stream can share
            # the compute stream's queue, which serialises the two)
            self.side = torch.cuda.Stream(priority=-1)
        return self.side

    def _use_slot(self, k):
        for n, t in self._slots[k].items():
            setattr(self, n, t)
        self._cur = k

    def _enable_slots(self):
        if self._slots is not None:
            return
        a = {n: getattr(self, n) for n in self.SLOT_ATTRS if getattr(self, n, None) is not None}
        depth = max(1, self.pf_depth)
        self._slots = [a] + [{n: torch.zeros_like(t) for n, t in a.items()} for _ in range(depth)]
        self._slot_free = [None] * len(self._slots)   # event: the compute stream is done with a set

    def prefetch(self, batch, graph=False):
        """Stage `batch` and build its index into an idle buffer set on the side stream;
        train_step(batch) then starts from it.  Up to pf_depth batches may be pending (buffer
        sets: pf_depth + 1), consumed in order.  graph=True replays the index build as a
        captured hipGraph (one per buffer set and batch size)."""
        self._enable_slots()
        if any(p[3] is batch for p in self._pfq) or len(self._pfq) >= len(self._slots) - 1:
            return
        cur = self._cur
        used = {cur} | {p[0] for p in self._pfq}
        k = next(i for i in range(len(self._slots)) if i not in used)
        side = self._side_stream()
        if self._slot_free[k] is not None:
            side.wait_event(self._slot_free[k])
        else:
            side.wait_stream(torch.cuda.current_stream())
        self._use_slot(k)
        try:
            with torch.cuda.stream(side):
                B = self.stage(batch)
                if graph:
                    key = (k, B, "pre")
                    g = self.graphs.get(key)
                    if g is None:
                        g = self.graphs[key] = self._capture(B, pre_only=True)
                    g.replay()
                else:
                    self._pre(B)
                ev = torch.cuda.Event()
                ev.record(side)
        finally:
            self._use_slot(cur)
        self._pfq.append((k, B, ev, batch))
        self._pf = self._pfq[0]

    def _begin(self, batch):
        """Buffers of this step's batch: the prefetched set if `batch` is the oldest one
        prefetched, else (every pending prefetch dropped once it lands) staged and indexed now
        on the compute stream."""
        q = self._pfq
        if q and batch is not None and batch is q[0][3]:
            k, B, ev, _ = q.pop(0)
            self._pf = q[0] if q else None
            self._use_slot(k)
            torch.cuda.current_stream().wait_event(ev)
            return B, True
        for p in q:      # other batches came: drop the prefetches (after they land)
            torch.cuda.current_stream().wait_event(p[2])
        if q:
            q.clear()
            self._pf = None
        return (self.stage(batch) if batch is not None else self.B), False

    def _step_mark(self, end):
        """bench.py (DLAMD_STEP_EVENTS=1): timing events on the compute stream around each step's
        launches — the step's own span, and the gap to the next step's start (waits included)."""
        ev = getattr(self, "step_events", None)
        if ev is not None:
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            ev.append((end, e))

    def _release(self):
        """Mark the current buffer set free once the compute stream's queued work is done."""
        if self._slots is not None:
            ev = torch.cuda.Event()
            ev.record()
            self._slot_free[self._cur] = ev

    def train_step(self, batch=None, graph=False, next_batch=None):
        """One training step on `batch` (or on the already-staged slots if None).
        next_batch: prefetch it (stage + index build on the side stream) during this step."""
        if self.bn and (self.B if batch is None else int(np.prod(np.shape(batch["label"])))) < 2:
            raise ValueError("batch_norm: a training batch needs at least 2 samples (the batch variance and its "
                             "unbiased factor B / (B - 1) are undefined at B = 1)")
        B, indexed = self._begin(batch)
        if self.p_plane is not None:   # predict's planes go stale: free them
            self.p_plane = self.w1_plane = None
            self.planes_step = -1
        if self.lazy:
            # every row's lag must stay below the alpha ring (rec.hip)
            if self.since_flush >= self.hist_len - 2:
                self.flush()
            self.since_flush += 1
        if not indexed and not graph:
            self._pre(B)
        # next_batch: the batch after this one, or a list of the next ones (up to pf_depth are
        # kept in flight), prefetched before this step's graph is submitted
        ahead = [] if next_batch is None else list(next_batch) if isinstance(next_batch, (list, tuple)) else [next_batch]
        for nb in ahead:
            self.prefetch(nb, graph=graph)
        self._step_mark(0)
        if graph:
            # one graph per (buffer set, batch size, index built inside or prefetched)
            key = (self._cur, B, not indexed)
            g = self.graphs.get(key)
            if g is None:
                g = self.graphs[key] = self._capture(B, with_pre=not indexed)
            g.replay()
        else:
            self._train(B)
        self._step_mark(1)
        self._release()
        self._queue_status()
        self.steps += 1
        self.last_batch = B
        return B

    def _embed_bwd_lazy(self, B, L, s):
        """The lazy-record embedding backward on stream s: every unique row's ordered
        segment sum and TF1 Adam step (dl_rec_bwd_adam), then the FM cont-field rows."""
        sp = self.spec
        bwd_blocks = call_int("dl_embed_bwd_grid", C_ref(L))
        E, R = sp.E, self.n_rep
        fn, fd = self._fm_bwd("dl_rec_bwd_adam")
        self._c("embed_bwd", fn, C_ref(L), ptr(self.rec), self.rec_ld, self.rec_flags, R,
                ptr(self.rows_u), ptr(self.rows_u1), ptr(self.mv_u), ptr(self.idx_uniq), ptr(self.idx_off),
                ptr(self.idx_n), ptr(self.idx_refs), 1, B * self.n_slot, ptr(self.dz), ptr(self.w_head),
                ptr(self.fm_sum), ptr(self.dx0), ptr(self.g_rep), ptr(self.g1_rep), ptr(self.hist),
                self.hist_len, ptr(self.opt), C_ref(self.pool_desc) if sp.M else None, ptr(self.hot_ws),
                self.hot_ws.numel(), *fd, s)
        if R:
            # FM cont-field rows: per-block register partials (on the blocks that hold samples),
            # folded into g_rep, then the rows updated
            cb = self._cont_blocks(B, bwd_blocks)
            fn, fd = self._fm_bwd("dl_embed_cont_bwd")
            self._c("cont_bwd", fn, C_ref(L), ptr(self.rows_u), ptr(self._cont()),
                    ptr(self.dz), ptr(self.w_head), ptr(self.fm_sum), ptr(self.cont_slab), cb, *fd, s)
            self._c("cont_reduce", "dl_embed_cont_reduce", C_ref(L), ptr(self.cont_slab), cb,
                    ptr(self.g_rep), ptr(self.g1_rep), ptr(self.rep_touched), s)
            self._c("adam_rep", "dl_rec_apply_rows", ptr(self.rec), self.rec_ld, E, self.rec_flags, sp.fm_cont_offset, R,
                    ptr(self.g_rep), ptr(self.g1_rep), ptr(self.hist), self.hist_len, ptr(self.opt), s)

    def _cont_blocks(self, B, bwd_blocks):
        """dl_embed_cont_bwd's blocks that hold samples (embed.hip cont_bwd_kernel: 16 samples a
        lane group, 64 / (E / 4) per wave, four waves): the rest would write zero partials."""
        spw = 64 // (self.spec.E // 4)
        return max(1, min(bwd_blocks, (B + 16 * spw - 1) // (16 * spw)))

    def _capture(self, B, with_pre=False, pre_only=False):
        """Capture the step (with its index build when `with_pre`), or only the index build
        (`pre_only`: the prefetch graph), on a capture stream; replayed on the caller's."""
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph()
        with capture_guard(), torch.cuda.graph(g, stream=s, capture_error_mode="thread_local"):
            if with_pre or pre_only:
                self._pre(B)
            if not pre_only:
                self._train(B)
        torch.cuda.current_stream().wait_stream(s)
        return g

    def predict(self, batch, logits=False, device=False):
        """Forward only: returns sigmoid scores [B] (or the logits) as host numpy, or as a
        device tensor (a copy) with device=True.  On a flushed table (no training step since
        the last flush) the first predict writes the p / first-order planes once (a flush
        that only copies: every row is caught up) and every later one reads them."""
        if (self.lazy and not self.spec.M and self.since_flush == 0 and type(self) is CTREngine
                and self.planes_step != self.steps and self.flat_planes):
            self.flush(planes=True)
        B, indexed = self._begin(batch)
        s = _lib.stream_handle()
        if not indexed:
            self._pre(B, weights=False)
        self._forward(B, s)
        self._release()
        self.check_error()
        out = (self.z if logits else self.score)[:B]
        return out.clone() if device else out.cpu().numpy()

    def loss(self):
        """Loss of the last training step: data term + the L2 terms on the pre-update
        weights (accumulated by the Adam kernels into opt[DL_OPT_REG], int64 fixed point)."""
        sp = self.spec
        H = sp.hidden[-1]
        B = self.last_batch
        width = self.head_slab.shape[1]
        rows = call_int(self.head_grid, B)
        data = self.head_slab[:rows, width - 1].double().sum().item()
        if self.weighted:   # sum w l / N_nz (0 when every weight is 0), N_nz from the device normaliser
            nz = float(self.norm[1].item())
            data = data / nz if nz else 0.0
        else:
            data = data / B
        if sp.hidden_reg == "l1":   # l1_regularizer: scale * sum |W| (dnn.py:88-90)
            return data + sp.l2 * _lib.reg_sum(self.opt)
        reg = _lib.reg_sum(self.opt)
        if self.wide_flushes:
            # the wide rows the step left untouched: their L2 term from a flush (wide.hip); the
            # touched rows' from the update's block partials — only the blocks this batch size
            # launched (a smaller last batch leaves an earlier batch's partials beyond them)
            self._wide_flush()
            nparts = int(_lib.lib().dl_wide_update_blocks(B * sp.Fw, H))
            reg += _lib.reg_sum(self.wsq) + float(self.wsq_part[:nparts].double().sum().item())
        return data + sp.l2 * 0.5 * reg

    def loss_sum_begin(self):
        """Start a running loss sum over the following training steps (the load-style fit's
        epoch loss, wdl.py:305-313): no host read per step — each step's graph adds its data and
        regulariser terms on the device (dl_loss_accumulate), and with lazy wide records their
        L2 term arrives as the records are applied (the wide table is flushed first, so every
        replayed step from here on belongs to the sum)."""
        if self.wide_flushes:
            self._wide_flush()
            self.wacc.zero_()
        self.loss_acc.zero_()

    def loss_sum_end(self):
        """(sum of the per-step losses since loss_sum_begin, steps): every wide record is caught
        up first, which adds the L2 terms of the steps it left untouched."""
        sp = self.spec
        acc = self.loss_acc.tolist()
        total = acc[0] + acc[1]
        if self.wide_flushes:
            self._wide_flush()
            total = (self.loss_acc[0] + self.loss_acc[1] + 0.5 * sp.l2 * self.wacc.sum()).item()
        return float(total), int(round(acc[2]))

    # ------------------------------------------------------------------ errors
    def _queue_status(self):
        """After each step: an asynchronous read-back of the status word into pinned host
        memory.  Completed read-backs are checked at the next steps without waiting; at most
        two may be outstanding, so a bad batch raises within two train_step calls (TF raises
        in the failing sess.run; here the failing step itself has applied nothing)."""
        if self._ring is not None:
            return self._ring_status()
        if self._status_host is None:
            self._status_host = torch.zeros(4, dtype=torch.int32, pin_memory=True)
        k = self.steps % 4
        self._status_host[k:k + 1].copy_(self.opt.view(torch.int32)[_lib.OPT_STATUS:_lib.OPT_STATUS + 1],
                                         non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self._status_q.append((k, ev))
        while self._status_q:
            k0, e0 = self._status_q[0]
            if len(self._status_q) > 2:
                t0 = time.perf_counter()
                e0.synchronize()
                self.host_wait += time.perf_counter() - t0   # bench.py: host time spent ahead of the GPU
            elif not e0.query():
                break
            self._status_q.pop(0)
            if int(self._status_host[k0]) != 0:
                self._status_q.clear()
                self.check_error()

    def _ring_status(self):
        """_queue_status from the status ring the step's last kernel writes (slot k & 3: the
        step sequence k and its status word): reports already written are checked without
        waiting; with more than two steps outstanding the oldest is waited for."""
        r = self._ring_np
        if self._ring_sent is None:   # first step: the device's sequence (this read waits for it)
            self._ring_sent = int(self.opt.view(torch.int32)[_lib.OPT_SEQ].item())
            self._ring_checked = self._ring_sent - 1
        else:
            self._ring_sent += 1
        while self._ring_checked < self._ring_sent:
            k = self._ring_checked + 1
            j = 2 * (k & 3)
            if int(r[j]) != k:
                if self._ring_sent - self._ring_checked <= 2:
                    break
                t0 = time.perf_counter()
                spins = 0
                while int(r[j]) != k:
                    spins += 1
                    if spins > 1000:   # past ~1 ms: yield the core instead of spinning on it
                        time.sleep(2e-5)
                    if time.perf_counter() - t0 > 10.0:   # the sequence went out of step: resynchronise
                        torch.cuda.synchronize()
                        if int(r[j]) != k:
                            self._ring_sent = None
                            self.check_error()
                            return
                self.host_wait += time.perf_counter() - t0   # bench.py: host time spent ahead of the GPU
            self._ring_checked = k
            if int(r[j + 1]) != 0:
                self.check_error()

    def set_opt(self, values):
        """Restore the optimizer block (a checkpoint's opt array) mid-process.  The step sequence
        of the status ring (opt[DL_OPT_SEQ]) belongs to this process's timeline, not the
        checkpoint's: the device's current value is kept, and the host re-reads it at the next
        step (otherwise the ring numbers the host expects would never arrive)."""
        v = torch.as_tensor(values, dtype=torch.float32).to(self.dev).clone()
        v[_lib.OPT_SEQ] = self.opt[_lib.OPT_SEQ]
        self.opt.copy_(v)
        if self._ring is not None:
            self._ring_sent = None

    def _error_words(self):
        words = [self.err]
        for sl in self._slots or []:
            if sl.get("err") is not None and sl["err"] is not self.err:
                words.append(sl["err"])
        return words

    def check_error(self):
        """Raise (and clear) a pending device error: out-of-range ids of any batch buffer set
        or the optimizer's status word."""
        st = self.opt.view(torch.int32)[_lib.OPT_STATUS:_lib.OPT_STATUS + 1]
        status = int(st.item())
        # the current buffer set's validation word: a batch validated whose step has not begun
        # (predict); a trained batch's word is consumed by its step (dl_step_begin -> status),
        # and every batch's own validation resets its word (no other set's word is touched:
        # a prefetched bad batch must still be skipped by its own step)
        errw = int(self.err[0].item())
        bad = errw != 0 and not status
        if not status and not bad:
            return
        bad_step, n_bad = (int(x) for x in self.opt[_lib.OPT_BAD_STEP:_lib.OPT_BAD_COUNT + 1].tolist())
        if bad:
            self.err.zero_()
        self.opt[_lib.OPT_STATUS:_lib.OPT_BAD_COUNT + 1].zero_()   # status, skip, bad step, count
        self._status_q.clear()
        if status & _lib.STATUS_LAG:
            raise _lib.DLError("internal: a row record lagged past the alpha ring (flush schedule)")
        if status & _lib.STATUS_INDEX:
            raise _lib.DLError("internal: batch index entry out of range (corrupt index)")
        if (status or errw) & _lib.STATUS_BAD_WEIGHT and not (status or errw) & _lib.STATUS_BAD_ID:
            raise _lib.DLError("InvalidArgumentError: sample weight negative, NaN or infinite (batch[\"weight\"] "
                               "must be finite and >= 0) — %s" % (
                                   "%d batch(es) skipped with no update, the last at global_step %d; the batches "
                                   "around them applied normally" % (n_bad, bad_step) if status else
                                   "in the current batch, no update applied"))
        if not status:   # a validated batch whose step has not begun yet (predict, or queued)
            raise _lib.DLError("InvalidArgumentError: categorical id out of range [0, %d) in the current "
                               "batch — no update applied" % self.N)
        raise _lib.DLError("InvalidArgumentError: categorical id out of range [0, %d) — %d batch(es) skipped "
                           "with no update, the last at global_step %d; the batches around them applied "
                           "normally" % (self.N, n_bad, bad_step))


def default_adam(spec):
    """Table Adam used by the drop-in model classes: row records with lazy-exact
    catch-up (bit-identical to the dense sweep, rec.hip) wherever supported."""
    return "lazy"


def _s3_dw_splits(M, N, B, base, cus=256):
    """Split-K slab count of one s3 weight gradient (dl_gemm_s3_tn: one 128 x 224 block per CU,
    (M / 128) x (N / 224) tiles per slab).  The blocks run in ceil(tiles x s / cus) rounds of
    ceil(B / s) batch rows (rounded to 64) each; the s <= base minimising rounds x rows, the
    largest on ties.  C2's layers (8 tiles) keep 32; C3's layer 0 (M = 528: 10 tiles) takes 25
    — one round of 250 blocks instead of two rounds for 320."""
    tiles = -(-M // 128) * -(-N // 224)

    def cost(s):
        return -(-tiles * s // cus) * (-(-(-(-B // s)) // 64) * 64)
    return min(range(base, 0, -1), key=cost)


@contextlib.contextmanager
def capture_guard():
    """No Python garbage collection while a hipGraph is being captured: a collection that
    frees an unreachable object holding a HIP resource (a torch.cuda.Event of an engine a
    caller dropped) would call hipEventDestroy inside the capture, which HIP refuses (the
    process aborts).  Garbage is collected before the capture instead."""
    enabled = gc.isenabled()
    gc.collect()
    gc.disable()
    try:
        yield
    finally:
        if enabled:
            gc.enable()


def _bf16_dw_splits(M, B, base, cus=256):
    """Split-K slab count of one bf16 weight gradient.  With whole 32-row batch steps
    (B % 32 == 0) dl_gemm_bf16 runs the LDS-DMA ring kernel: one 144 x 400 block per CU,
    ceil(M / 144) tiles per slab; the s <= base minimising rounds x rows per block, the largest
    on ties (C5: M = 432 / 416 -> 3 tiles, 79 slabs of 832 rows, 237 blocks in one round).
    Otherwise the two-buffer kernel (64-row tiles, two blocks per CU) takes `base`."""
    if B % 32:
        return base
    tiles = -(-M // 144)

    def cost(s):
        return -(-tiles * s // cus) * (-(-(-(-B // s)) // 64) * 64)
    return min(range(base, 0, -1), key=cost)


def _num_splits(K, splits, align=16):
    """Split-K slabs the GEMM actually writes (K chunks rounded up to `align`: 16 for the f32
    kernel, 64 for the bf16 fast kernel)."""
    kps = -(-K // splits)
    kps = -(-kps // align) * align
    return -(-K // kps)


def call_int(name, *args):
    return getattr(_lib.lib(), name)(*args)


def C_ref(L):
    import ctypes
    return ctypes.byref(L)


def _copy_in(dst, x, dtype, dev):
    """One input array into its static device slot: a pinned host tensor of the slot's dtype is
    copied straight in, asynchronously on the current stream (no host wait); anything else goes
    through _as_dev."""
    if isinstance(x, torch.Tensor) and not x.is_cuda and x.dtype == dtype and x.is_pinned():
        dst.copy_(x.view(dst.shape), non_blocking=True)
    else:
        dst.copy_(_as_dev(x, dtype, dev).reshape(dst.shape))


def _as_dev(x, dtype, dev):
    if isinstance(x, torch.Tensor):
        return x.to(device=dev, dtype=dtype, non_blocking=True)
    return torch.from_numpy(np.ascontiguousarray(x)).to(device=dev, dtype=dtype, non_blocking=True)
