"""GPU check of the side options' descriptor table (deep_learning_amd/branches.py) with every option on at once:
the launches of one training step and one predict, label and entry point each, against the list the engine
issued when every branch was still written out by hand; the logit chain's threading (every member's z_in is
the member before's z_out, the head's extra logit the last one's); and initial parameters that depend on the
seed alone."""
import ctypes

import numpy as np
import pytest
import torch

from deep_learning_amd.engine import CTREngine, ModelSpec
from tests import _cross_ref as X

pytestmark = pytest.mark.gpu

NAME = "dnn_pipeline"
KW = dict(C=13, V=3, S=8, E=8, cate_index_size=3000, hidden=[32, 16])
B_ = 64
CHAIN = ["cross", "afm", "ccpm", "cin", "autoint"]
ALL = dict(cross_layers=2, afm_attention=4, ccpm_filters=(2, 2), cin_layers=(3, 2), autoint_layers=1, autoint_heads=2,
           autoint_dim=8, bi_interaction=True)

FRONT = [("rec_gather", "dl_rec_gather"), ("embed_fwd", "dl_embed_fwd_indexed"), ("bi_fwd", "dl_bi_fwd")]
CHAIN_FWD = [(k + "_fwd", "dl_%s_fwd" % k) for k in CHAIN] + [("head", "dl_head_fwd_bwd_cross")]
CHAIN_BWD = [(k + "_bwd", "dl_%s_bwd" % k) for k in CHAIN]
CHAIN_ADAM = [("adam_head", "dl_adam_dense")] + [("adam_" + k, "dl_adam_dense") for k in CHAIN]
TOWER_PNN = [("gemm_fwd_l0", "dl_gemm_s3_nt_bits"), ("pnn_fwd", "dl_pnn_inner_fwd"), ("gemm_fwd_l1", "dl_gemm_s3_nt_bits")]
TOWER_BN = [("gemm_fwd_l0", "dl_gemm_s3_nt_bits"), ("bn_stats_l0", "dl_bn_stats"), ("bn_fwd_l0", "dl_bn_fwd"),
            ("gemm_fwd_l1", "dl_gemm_s3_nt_bits"), ("bn_stats_l1", "dl_bn_stats"), ("bn_fwd_l1", "dl_bn_fwd")]
PRE = [("validate", "dl_validate_batch"), ("index_build", "dl_index_build")]
# tag -> (the options, one training step's launches, one predict's)
CONFIGS = {
    "pnn": (dict(ALL, pnn="inner"),
            PRE + [("step_begin", "dl_step_begin")] + FRONT + TOWER_PNN + CHAIN_FWD
            + [("gemm_dw_l1", "dl_gemm_s3_tn"), ("gemm_dx_l1", "dl_gemm_s3_nt_bits"), ("gemm_dw_l0", "dl_gemm_s3_tn"),
               ("gemm_dx_l0", "dl_gemm_s3_nt"), ("adam_dense", "dl_adam_dense_layers")]
            + CHAIN_BWD + [("pnn_bwd", "dl_pnn_inner_bwd"), ("bi_bwd", "dl_bi_bwd"), ("embed_bwd", "dl_rec_bwd_adam")]
            + CHAIN_ADAM + [("adam_pnn", "dl_adam_dense"), ("loss_acc", "dl_loss_accumulate")],
            PRE + FRONT + TOWER_PNN + CHAIN_FWD),
    "bn": (dict(ALL, batch_norm=True),
           PRE + [("step_begin", "dl_step_begin")] + FRONT + TOWER_BN + CHAIN_FWD
           + [("bn_sums_l1", "dl_bn_bwd_sums"), ("bn_apply_l1", "dl_bn_bwd_apply"), ("gemm_dw_l1", "dl_gemm_s3_tn"),
              ("bn_bias_l1", "dl_bn_zero_bias_grad"), ("gemm_dx_l1", "dl_gemm_s3_nt_bits"),
              ("bn_sums_l0", "dl_bn_bwd_sums"), ("bn_apply_l0", "dl_bn_bwd_apply"), ("gemm_dw_l0", "dl_gemm_s3_tn"),
              ("bn_bias_l0", "dl_bn_zero_bias_grad"), ("gemm_dx_l0", "dl_gemm_s3_nt"),
              ("adam_dense", "dl_adam_dense_layers")]
           + CHAIN_BWD + [("bi_bwd", "dl_bi_bwd"), ("embed_bwd", "dl_rec_bwd_adam"), ("adam_bn_l0", "dl_adam_dense"),
                          ("adam_bn_l1", "dl_adam_dense")]
           + CHAIN_ADAM + [("loss_acc", "dl_loss_accumulate")],
           PRE + FRONT + [t for t in TOWER_BN if "stats" not in t[0]] + CHAIN_FWD),
}


def _pointers(args):
    return [a.value for a in args if isinstance(a, ctypes.c_void_p)]


def _threading(calls):
    """Every chain member's logit is its last pointer before the stream; the next member reads it."""
    fwd = [(label, args) for label, _, args in calls if label.endswith("_fwd") and label[:-4] in CHAIN]
    assert [label[:-4] for label, _ in fwd] == CHAIN
    z_prev = None
    for label, args in fwd:
        assert isinstance(args[-2], ctypes.c_void_p) and args[-2].value, label
        if label == "cross_fwd":
            assert None not in args, label                       # no z_in argument at all
        elif label == "afm_fwd":
            assert args[-4].value == z_prev, label
        else:
            assert args[-3].value == z_prev, label
        z_prev = args[-2].value
    head = [args for label, _, args in calls if label == "head"]
    assert len(head) == 1 and z_prev in _pointers(head[0])


@pytest.mark.parametrize("tag", list(CONFIGS))
def test_launch_sequence_and_seeded_parameters(hip_lib, monkeypatch, tag):
    opts, step, predict = CONFIGS[tag]
    calls = []
    orig = CTREngine._c

    def spy(self, label, name, *args):
        calls.append((label, name, args))
        return orig(self, label, name, *args)

    monkeypatch.setattr(CTREngine, "_c", spy)
    eng = CTREngine(ModelSpec(NAME, **opts, **KW), max_batch=B_, seed=5, adam="lazy")
    eng.train_step(X.make_batch(NAME, KW, B_, 70))
    torch.cuda.synchronize()
    assert [c[:2] for c in calls] == step
    _threading(calls)
    del calls[:]
    eng.predict(X.make_batch(NAME, KW, B_, 71))
    eng.check_error()
    assert [c[:2] for c in calls] == predict
    _threading(calls)
    Pa, Pb = (CTREngine(ModelSpec(NAME, **opts, **KW), max_batch=B_, seed=5, adam="lazy").params() for _ in range(2))
    assert set(Pa) == set(Pb) and any(k.startswith("autoint_") for k in Pa)
    for k in Pa:
        np.testing.assert_array_equal(Pa[k], Pb[k], err_msg=k)
