"""FTRL-proximal for the wdl wide weights (ModelSpec.wide_optimizer = "ftrl"), the parts that
need no GPU: the float64 restatement (tests/_ftrl_ref.py) against the oracle and against a direct
transcription of TF's ApplyFtrl, the spec, local_run's overrides and the refusals."""
import math
import types

import numpy as np
import pytest

from oracle import ctr_ref as R
from tests import _ftrl_ref as FR

KW = dict(C=3, S=4, E=8, cate_index_size=50, hidden=[16, 8], Fw=3)


def test_restatement_is_the_oracle_wdl():
    """With the reference's L2 term on wdl_weights kept, the torch float64 forward / backward is
    oracle.ctr_ref's wdl forward / backward run in float64 (analytic gradients), to rounding."""
    cfg = R.make_cfg("wdl", **KW)
    P = R.init_params(cfg, np.random.default_rng(5))
    b = FR.make_batch(KW, 63, seed=1)
    assert np.isin(b["wide_feats"], np.arange(KW["Fw"], KW["Fw"] + 8)).any()      # ids aliasing deep-output rows
    assert np.unique(b["wide_feats"]).size < b["wide_feats"].size                 # ids repeated in the batch
    fw = R.forward(cfg, P, b, dtype=np.float64)
    G, _ = R.backward(cfg, P, b, fw, dtype=np.float64)
    fb = FR.forward_backward(cfg, P, b, wide_l2=True)
    assert np.abs(fb["z"] - fw["z"]).max() < 1e-12
    assert abs(fb["loss"] - fw["loss"]) < 1e-12
    for k in P:
        assert np.abs(fb["G"][k] - G[k]).max() < 1e-12, k
    # without the wide L2 term only the wdl_weights gradient and the loss change, by l2 w and l2/2 sum w^2
    fn = FR.forward_backward(cfg, P, b)
    w = P["wdl_weights"].astype(np.float64)
    assert np.abs(fn["G"]["wdl_weights"] + cfg.l2 * w - G["wdl_weights"]).max() < 1e-12
    assert abs(fn["loss"] + cfg.l2 * 0.5 * (w ** 2).sum() - fw["loss"]) < 1e-12
    for k in P:
        if k != "wdl_weights":
            assert np.abs(fn["G"][k] - G[k]).max() < 1e-12, k


def _apply_ftrl_tf(var, accum, linear, grad, lr, l1, l2):
    """training_ops.cc ApplyFtrl (FtrlCompute, learning_rate_power = -0.5, no shrinkage), one
    scalar, transcribed statement by statement."""
    new_accum = accum + grad * grad
    linear += grad - (math.sqrt(new_accum) - math.sqrt(accum)) / lr * var
    quadratic = math.sqrt(new_accum) / lr + 2.0 * l2
    l1_reg_adjust = max(min(linear, l1), -l1)            # clip(linear, -l1, l1)
    var = (l1_reg_adjust - linear) / quadratic          # 0 exactly where |linear| <= l1
    return var, new_accum, linear


@pytest.mark.parametrize("w,z,n,g,lr,l1,l2", [
    (0.3, 0.0, 0.1, 0.02, 0.05, 0.0, 0.0),        # l1 = 0
    (0.3, 0.0, 0.1, 0.02, 0.05, 0.0, 0.7),        # l2 > 0
    (0.3, 0.0, 0.1, 0.002, 0.05, 0.01, 0.0),      # |z'| <= l1 -> exactly 0
    (-0.2, 0.05, 0.4, -0.3, 0.05, 0.01, 0.1),     # |z'| > l1, negative side
    (0.0, -0.02, 0.1, 0.0, 0.1, 0.01, 0.0),       # g = 0 on a touched row: w recomputed from z
    (0.1, 0.01, 0.1, 0.0, 0.1, 0.01, 0.0),        # |z'| == l1 -> 0 (the comparison is strict)
])
def test_ftrl_step_is_tf_apply_ftrl(w, z, n, g, lr, l1, l2):
    wv, zv, nv, gv = (np.array([x], np.float64) for x in (w, z, n, g))
    FR.ftrl_apply(wv, zv, nv, gv, [0], lr, l1, l2)
    ew, en, ez = _apply_ftrl_tf(w, n, z, g, lr, l1, l2)
    assert abs(wv[0] - ew) < 1e-15 and abs(zv[0] - ez) < 1e-15 and abs(nv[0] - en) < 1e-15
    if abs(ez) <= l1:
        assert wv[0] == 0.0 and ew == 0.0


def test_duplicate_ids_are_summed_once():
    """A row referenced k times in a batch takes one step on the summed gradient
    (_apply_sparse_duplicate_indices), not k steps; untouched rows keep their bits."""
    cfg = R.make_cfg("wdl", **KW)
    P = R.init_params(cfg, np.random.default_rng(6))
    b = FR.make_batch(KW, 16, seed=2, id_hi=30, hot=20)      # id 20 in every sample (not a deep-output row)
    ref = FR.FtrlRef(cfg, P, lr=0.05, l1=0.0, l2=0.0)
    w0 = ref.w.copy()
    fw = ref.train_step(b)
    g = fw["G"]["wdl_weights"][20, 0]
    assert (np.asarray(b["wide_feats"]) == 20).sum() >= 16
    ew, en, ez = _apply_ftrl_tf(float(w0[20]), FR.N0, 0.0, float(g), 0.05, 0.0, 0.0)
    assert abs(ref.w[20] - ew) < 1e-15 and abs(ref.n[20] - en) < 1e-15 and abs(ref.z[20] - ez) < 1e-15
    rows = FR.touched_rows(b, 8)
    rest = np.setdiff1d(np.arange(w0.size), rows)
    assert rest.size and np.array_equal(ref.w[rest], w0[rest])
    assert np.all(ref.z[rest] == 0.0) and np.all(ref.n[rest] == FR.N0)
    assert set(range(KW["Fw"], KW["Fw"] + 8)) <= set(rows.tolist())     # the deep-output rows: always touched


def test_spec_defaults_and_values():
    from deep_learning_amd.engine import ModelSpec
    sp = ModelSpec("wdl", **KW)
    assert (sp.wide_optimizer, sp.wide_lr, sp.wide_l1, sp.wide_l2) == ("adam", None, 0.0, 0.0)
    sp = ModelSpec("wdl", wide_optimizer="ftrl", lr=0.002, **KW)
    assert sp.wide_lr is None and sp.ftrl_lr == 0.002          # None: the model's learning rate
    sp = ModelSpec("wdl", wide_optimizer="ftrl", wide_lr=0.05, wide_l1=1e-3, wide_l2=0.5, **KW)
    assert (sp.ftrl_lr, sp.wide_l1, sp.wide_l2) == (0.05, 1e-3, 0.5)


@pytest.mark.parametrize("model", ["deepfm_pipeline", "dnn_pipeline", "deepfm_multi", "dnn", "deepfm"])
def test_spec_refuses_other_models(model):
    from deep_learning_amd.engine import ModelSpec
    with pytest.raises(ValueError, match="wide_optimizer"):
        ModelSpec(model, wide_optimizer="ftrl")
    assert ModelSpec(model, wide_optimizer="adam").wide_optimizer == "adam"


@pytest.mark.parametrize("bad", [dict(wide_optimizer="adagrad"), dict(wide_lr=0.0), dict(wide_lr=-0.1),
                                 dict(wide_lr=float("nan")), dict(wide_lr=float("inf")), dict(wide_l1=-1e-3),
                                 dict(wide_l1=float("inf")), dict(wide_l2=-1.0), dict(wide_l2=float("nan"))])
def test_spec_refuses_bad_values(bad):
    from deep_learning_amd.engine import ModelSpec
    with pytest.raises(ValueError, match="wide_optimizer"):
        ModelSpec("wdl", **dict(dict(wide_optimizer="ftrl"), **bad), **KW)


def test_sharded_engine_refuses():
    """Before anything touches a device or the exchange."""
    from deep_learning_amd.engine import ModelSpec
    from deep_learning_amd.shard import ShardedCTREngine
    ex = types.SimpleNamespace(world=1, rank=0)
    with pytest.raises(ValueError, match="wide_optimizer"):
        ShardedCTREngine(ModelSpec("wdl", wide_optimizer="ftrl", **KW), 64, ex)


def _argv(tmp_path, alg, *over):
    conf = tmp_path / "conf"
    if not conf.exists():
        conf.mkdir()
        lines = ["f%d\tx\tfloat" % i for i in range(13)] + ["c%d\tx\tstring" % i for i in range(26)]
        (conf / "dnn.conf").write_text("\n".join(lines) + "\n")
    return ["local_run.py", alg, "train", "1", "8", "3000", "3", str(conf), "tr/", "pr/", "pb", "ck", "0", "ck",
            "batch_size=64"] + list(over)


def test_local_run_overrides(tmp_path):
    """The four overrides are parsed when given and absent from ModelParams.__dict__ (the
    start-up dump) when not; models/wdl.py passes them on to its ModelSpec."""
    from deep_learning_amd.local_run import ModelParams
    from deep_learning_amd.models.wdl import DeepModel
    plain = ModelParams(_argv(tmp_path, "wdl"))
    assert not {"wide_optimizer", "wide_lr", "wide_l1", "wide_l2"} & set(plain.__dict__)
    mp = ModelParams(_argv(tmp_path, "wdl", "wide_optimizer=ftrl", "wide_lr=0.05", "wide_l1=1e-3", "wide_l2=0"))
    assert (mp.wide_optimizer, mp.wide_lr, mp.wide_l1, mp.wide_l2) == ("ftrl", 0.05, 1e-3, 0.0)
    assert set(mp.__dict__) - set(plain.__dict__) == {"wide_optimizer", "wide_lr", "wide_l1", "wide_l2"}
    assert {k: v for k, v in mp.__dict__.items() if k in plain.__dict__} == plain.__dict__
    assert ModelParams(_argv(tmp_path, "dnn_pipeline", "wide_optimizer=adam")).wide_optimizer == "adam"

    def args(**kw):
        return types.SimpleNamespace(hidden_units=[16, 8], epochs=1, batch_size=64, learning_rate=0.001, model_pb="pb",
                                     l2_reg=1e-5, cont_field_size=3, cate_field_size=4, cate_index_size=50,
                                     embedding_size=8, wide_field_size=3, learning_rate_decay_steps=1000,
                                     learning_rate_decay_rate=0.9, **kw)
    sp = DeepModel(args(wide_optimizer=mp.wide_optimizer, wide_lr=mp.wide_lr, wide_l1=mp.wide_l1,
                        wide_l2=mp.wide_l2)).spec
    assert (sp.wide_optimizer, sp.ftrl_lr, sp.wide_l1, sp.wide_l2) == ("ftrl", 0.05, 1e-3, 0.0)
    assert DeepModel(args()).spec.wide_optimizer == "adam"


@pytest.mark.parametrize("alg,kv", [("wdl", "wide_optimizer=sgd"), ("dnn_pipeline", "wide_optimizer=ftrl"),
                                    ("wdl", "wide_lr=0"), ("wdl", "wide_lr=-1"), ("wdl", "wide_lr=abc"),
                                    ("wdl", "wide_lr=nan"), ("wdl", "wide_l1=-0.1"), ("wdl", "wide_l2=inf"),
                                    ("wdl", "wide_l2=")])
def test_local_run_refuses_bad_values(tmp_path, alg, kv):
    from deep_learning_amd.local_run import ModelParams
    with pytest.raises((SystemExit, ValueError), match="wide_optimizer"):
        ModelParams(_argv(tmp_path, alg, kv))
