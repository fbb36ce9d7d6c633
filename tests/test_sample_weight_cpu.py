"""CPU checks of sample weighting: local_run's pos_weight= / weight_key= options, the
refusals, the float64 reference (tests/_sample_weight_ref.py) against torch.autograd, and the
TFRecord weight column through the native reader."""
import os
import types

import numpy as np
import pytest
import torch

from tests import _sample_weight_ref as W


def _argv(tmp_path, *over):
    conf = tmp_path / "conf"
    if not conf.exists():
        conf.mkdir()
        lines = ["f%d\tx\tfloat" % i for i in range(13)] + ["c%d\tx\tstring" % i for i in range(26)]
        (conf / "dnn.conf").write_text("\n".join(lines) + "\n")
    return ["local_run.py", "deepfm_pipeline", "train", "1", "8", "3000", "3", str(conf), "tr/", "pr/", "pb", "ck",
            "0", "ck", "batch_size=64"] + list(over)


def test_model_params_parses_weight_options(tmp_path):
    from deep_learning_amd.local_run import ModelParams
    mp = ModelParams(_argv(tmp_path, "pos_weight=2.5", "weight_key=imp_w"))
    assert mp.pos_weight == 2.5 and mp.weight_key == "imp_w"
    mp = ModelParams(_argv(tmp_path, "pos_weight=0.25"))
    assert mp.pos_weight == 0.25 and not hasattr(mp, "weight_key")
    mp = ModelParams(_argv(tmp_path, "weight_key=w"))
    assert mp.weight_key == "w" and not hasattr(mp, "pos_weight")


def test_model_params_keys_unchanged_without_the_options(tmp_path):
    """The start-up dump prints ModelParams.__dict__: without the options it is what it was, and
    the options add exactly their own keys."""
    from deep_learning_amd.local_run import ModelParams
    plain = ModelParams(_argv(tmp_path))
    other = ModelParams(_argv(tmp_path, "learning_rate=0.01"))
    assert list(plain.__dict__) == list(other.__dict__)
    assert "pos_weight" not in plain.__dict__ and "weight_key" not in plain.__dict__
    both = ModelParams(_argv(tmp_path, "pos_weight=3", "weight_key=w"))
    assert set(both.__dict__) - set(plain.__dict__) == {"pos_weight", "weight_key"}
    assert {k: v for k, v in both.__dict__.items() if k in plain.__dict__} == plain.__dict__


@pytest.mark.parametrize("v", ["0", "-1", "nan", "inf", "-inf", "abc"])
def test_pos_weight_refused(tmp_path, v):
    from deep_learning_amd.engine import ModelSpec
    from deep_learning_amd.local_run import ModelParams
    with pytest.raises((SystemExit, ValueError), match="pos_weight"):
        ModelParams(_argv(tmp_path, "pos_weight=" + v))
    if v != "abc":
        with pytest.raises(ValueError, match="pos_weight"):
            ModelSpec("deepfm_pipeline", pos_weight=float(v))
    with pytest.raises((SystemExit, ValueError), match="weight_key"):
        ModelParams(_argv(tmp_path, "weight_key="))


def test_spec_and_model_pass_the_options_through():
    from deep_learning_amd.engine import ModelSpec
    from deep_learning_amd.models._ctr_model import _spec_from_args
    assert ModelSpec("deepfm_pipeline").pos_weight == 1.0
    args = types.SimpleNamespace(embedding_size=8, cate_feats_size=100, hidden_units=[8], learning_rate=1e-3,
                                 l2_reg=1e-5, learning_rate_decay_steps=10, learning_rate_decay_rate=0.9,
                                 cate_field_size=4, cont_field_size=2)
    assert _spec_from_args("deepfm_pipeline", args).pos_weight == 1.0
    args.pos_weight = 2.5
    assert _spec_from_args("deepfm_pipeline", args).pos_weight == 2.5


def test_sharded_engine_refuses():
    """Before anything touches a device or the exchange: both options, by name."""
    from deep_learning_amd.engine import ModelSpec
    from deep_learning_amd.shard import ShardedCTREngine
    pk = dict(C=13, S=26, E=8, cate_index_size=3000, hidden=[40, 24])
    ex = types.SimpleNamespace(world=1, rank=0)
    with pytest.raises(ValueError, match="sample_weight.*pos_weight"):
        ShardedCTREngine(ModelSpec("deepfm_pipeline", **pk), 64, ex, sample_weight=True)
    with pytest.raises(ValueError, match="sample_weight.*pos_weight"):
        ShardedCTREngine(ModelSpec("deepfm_pipeline", pos_weight=2.0, **pk), 64, ex)


def test_effective_weights_and_normaliser():
    y = np.float32([1, 0, 1, 0, 1, 0])
    w = np.float32([1, 1, 0, 0.5, 3, 0])
    we, nz, inv, bad = W.w_eff_f32(w, y, 2.5)
    np.testing.assert_array_equal(we, np.float32([2.5, 1, 0, 0.5, 7.5, 0]))
    assert (nz, bad) == (4, False) and inv == np.float32(0.25)
    we, nz, inv, bad = W.w_eff_f32(None, y, 1.0)
    np.testing.assert_array_equal(we, np.ones(6, np.float32))
    assert nz == 6 and inv == np.float32(1.0 / 6)
    assert W.w_eff_f32(np.zeros(6), y, 2.0)[1:3] == (0, np.float32(0))
    for v in (-1.0, np.nan, np.inf):
        w2 = w.copy()
        w2[1] = v
        we, nz, _, bad = W.w_eff_f32(w2, y, 2.5)
        assert bad and we[1] == 0 and nz == 3


@pytest.mark.parametrize("case", ["random", "zeros", "ones"])
def test_reference_matches_autograd_fp64(case):
    """loss64 / dz64 / head64 against torch.autograd on the SUM_BY_NONZERO_WEIGHTS loss written
    out in float64: value and gradients to 1e-12."""
    rng = np.random.default_rng(5)
    B, n, eps = 67, 19, 1e-7
    feat = rng.standard_normal((B, n))
    wh = rng.standard_normal(n) * 0.3
    y = (rng.random(B) < 0.3).astype(np.float64)
    w = {"random": rng.choice([0, 0.5, 1, 3], B).astype(np.float64) * (1 + 1.5 * y), "zeros": np.zeros(B),
         "ones": np.ones(B)}[case]
    ft, wt = torch.tensor(feat, requires_grad=True), torch.tensor(wh, requires_grad=True)
    bt = torch.tensor(0.1, dtype=torch.float64, requires_grad=True)
    p = torch.sigmoid(ft @ wt + bt)
    yt, wgt = torch.tensor(y), torch.tensor(w)
    per = -yt * torch.log(p + eps) - (1 - yt) * torch.log(1 - p + eps)
    nz = int((wgt != 0).sum())
    loss = (wgt * per).sum() / nz if nz else (wgt * per).sum() * 0.0
    loss.backward()
    ref = W.head64(feat, wh, 0.1, y, w, eps)
    assert abs(ref["loss"] - float(loss.detach())) < 1e-12
    np.testing.assert_allclose(ref["dfeat"], ft.grad.numpy(), atol=1e-12, rtol=0)
    np.testing.assert_allclose(ref["dw"], wt.grad.numpy(), atol=1e-12, rtol=0)
    assert abs(ref["db"] - float(bt.grad)) < 1e-12
    if case == "ones":     # the unweighted mean, the oracle's form
        assert abs(ref["loss"] - W.per_sample_loss(ref["p"], y, eps).mean()) < 1e-15
    if case == "zeros":
        assert ref["loss"] == 0 and not ref["dz"].any()


def test_weighted_oracle_step_is_the_plain_step_for_unit_weights():
    from deep_learning_amd.synthetic import make_batch
    from oracle import ctr_ref as R
    kw = dict(C=13, S=8, E=8, cate_index_size=2000, hidden=[16, 8])
    cfg = R.make_cfg("deepfm_pipeline", **kw)
    b = make_batch(32, cate_fields=8, cate_index_size=2000, seed=1)
    Pa = R.init_params(cfg, np.random.default_rng(0))
    Pb = {k: v.copy() for k, v in Pa.items()}
    fa = R.train_step(cfg, Pa, R.AdamTF1(cfg, Pa), b)
    fb = W.train_step(cfg, Pb, R.AdamTF1(cfg, Pb), dict(b, weight=np.ones(32, np.float32)))
    # the oracle rounds every sample's loss term to float32 (half an ulp, 6e-8 relative, of terms
    # below ~3) before its float64 mean; the restatement keeps them in float64
    assert abs(fa["loss"] - fb["loss"]) < 2e-7
    for k in Pa:
        np.testing.assert_allclose(Pa[k], Pb[k], atol=1e-7, rtol=0, err_msg=k)
    assert R.dlogit.__module__ == "oracle.ctr_ref"       # the oracle is left as it was


def test_reference_eval_stats():
    st = W.eval_stats([1, 0, 1, 0], np.float32([1.0, 0.0, 0.5, 0.25]), [2, 0, 1, 1])
    want = -(2 * np.log(1 + 1e-7) + np.log(0.5 + 1e-7) + np.log(0.75 + 1e-7)) / 4
    assert abs(st["logloss"] - want) < 1e-15
    assert st["calibration"] == 2.75 / 3 and st["weight_sum"] == 4 and st["n_nonzero"] == 3 and st["n"] == 4
    assert np.isnan(W.eval_stats([1, 0], [0.5, 0.5], [0, 0])["logloss"])


class _MP:
    def __init__(self, **kw):
        self.__dict__.update(dict(alg_name="deepfm_pipeline", epochs=1, batch_size=16, cont_field_size=13,
                                  vector_feats_size=2, cate_field_size=26, multi_feats_size=0, shuffle=0,
                                  shuffle_seed=None))
        self.__dict__.update(kw)


def test_tfrecord_weight_key_round_trip(tmp_path):
    """weight_key=NAME: the float [1] feature NAME arrives as batch["weight"]; without the option the
    reader's spec and batches are what they were; a record without the feature is refused."""
    from deep_learning_amd.synthetic import make_batch
    from deep_learning_amd.utils import data_loader
    b = make_batch(40, vector=2, cate_index_size=5000, seed=3)
    b["imp_w"] = np.random.default_rng(0).choice([0, 0.5, 1, 3], (40, 1)).astype(np.float32)
    data_loader.write_tfrecord_part(os.path.join(str(tmp_path), "part-00000"), b)
    files = data_loader.get_file_list(str(tmp_path) + "/")
    plain = list(data_loader.pipeline_process(_MP(), files, "pred"))
    assert set(plain[0]) == {"label", "cont_feats", "vector_feats", "cate_feats"}
    got = list(data_loader.pipeline_process(_MP(weight_key="imp_w"), files, "pred"))
    assert len(got) == 2 and set(got[0]) == set(plain[0]) | {"weight"}
    assert got[0]["weight"].shape == (16, 1) and got[0]["weight"].dtype == np.float32
    np.testing.assert_array_equal(np.concatenate([g["weight"] for g in got]), b["imp_w"][:32])
    np.testing.assert_array_equal(got[1]["cate_feats"], plain[1]["cate_feats"])
    with pytest.raises(ValueError):
        list(data_loader.pipeline_process(_MP(weight_key="absent"), files, "pred"))
    with pytest.raises(ValueError, match="weight_key"):
        data_loader.pipeline_process(_MP(weight_key="label"), files, "pred")


def test_eval_accumulator_wants_weights_for_every_batch_or_none():
    from deep_learning_amd.models._ctr_model import _wants_weights
    assert _wants_weights(["logloss"]) and _wants_weights(["gauc", "calibration"]) and not _wants_weights(["gauc"])
