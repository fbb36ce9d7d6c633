"""CPU checks of the inner-product layer (ModelSpec.pnn): the float64 restatement
(tests/_pnn_ref.py) pinned to the oracle at pnn = None, pnn_fwd64 against a literal transcription of
PNN.py:78-83, pnn_bwd64 against autograd and central differences, the 0-at-zero rule, ModelSpec's
and the sharded engine's refusals and local_run's pnn= override."""
import types

import numpy as np
import pytest
import torch

from oracle import ctr_ref as R
from tests import _pnn_ref as Pn

KW = {"dnn_pipeline": dict(C=5, V=3, S=6, E=8, cate_index_size=300, hidden=[16, 8]),
      "dnn_cate": dict(V=2, S=6, E=8, cate_index_size=300, hidden=[16, 8]),
      "dnn_multi": dict(C=5, V=2, S=4, E=8, cate_index_size=300, hidden=[16, 8],
                        multi_ranges=[[0, 7, "a"], [7, 12, "b"]]),
      "dnn_multi_cate": dict(V=0, S=4, E=8, cate_index_size=300, hidden=[16, 8],
                             multi_ranges=[[0, 5, "a"], [5, 6, "b"]])}


@pytest.mark.parametrize("name", list(KW))
def test_restatement_is_the_oracle_without_the_layer(name):
    """pnn = None: logits, loss and every parameter gradient equal ctr_ref.forward /
    ctr_ref.backward run in float64, to float64 rounding."""
    kw = KW[name]
    cfg = R.make_cfg(name, **kw)
    P = Pn.init_params(cfg, 0, 0, False, np.random.default_rng(3))
    assert set(P) == set(R.init_params(cfg, np.random.default_rng(3)))
    b = Pn.X.make_batch(name, kw, 37, 5)
    got = Pn.forward_backward(cfg, P, b)
    fw = R.forward(cfg, P, b, dtype=np.float64)
    G, _ = R.backward(cfg, P, b, fw, dtype=np.float64)
    np.testing.assert_allclose(got["z"], fw["z"], rtol=1e-12, atol=1e-14)
    assert abs(got["loss"] - fw["loss"]) < 1e-13
    for k in P:
        scale = np.abs(G[k]).max()
        assert scale > 0, k
        np.testing.assert_allclose(got["G"][k], G[k], rtol=0, atol=1e-12 * scale, err_msg=k)


def _point(F, E, D1, seed, B=4):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((B, F, E)), rng.standard_normal((D1, F)), rng.standard_normal((B, D1))


@pytest.mark.parametrize("F,E,D1", [(2, 8, 1), (3, 4, 5), (7, 8, 3)])
def test_forward_is_the_reference_lines(F, E, D1):
    """pnn_fwd64 equals PNN.py:78-83 written out: per hidden unit, the fields multiplied by theta's
    row, reduced over the fields, and the norm over the embedding axis."""
    x, theta, _ = _point(F, E, D1, 10 * F + D1)
    lp, T = Pn.pnn_fwd64(x, theta)
    want = []
    for i in range(D1):
        th = theta[i].reshape(1, F, 1)                   # tf.reshape(theta, (1, num_inputs, 1))
        delta = (x * th).sum(1)                          # tf.reduce_sum(tf.multiply(embed, theta), 1)
        want.append(np.sqrt((delta ** 2).sum(1)))        # tf.norm(., axis=1)
    np.testing.assert_allclose(lp, np.stack(want, 1), rtol=1e-13, atol=0)
    assert T.shape == (4, D1, E)


@pytest.mark.parametrize("F,E,D1", [(2, 8, 1), (3, 4, 5), (7, 8, 3)])
def test_backward_formulas_match_autograd_and_finite_differences(F, E, D1):
    """pnn_bwd64 against torch autograd of sum r lp (1e-10 relative) and against central differences
    with step 1e-6, the fixture's smallest lp asserted far above the step first."""
    x, theta, r = _point(F, E, D1, 100 * F + D1)
    lp, _ = Pn.pnn_fwd64(x, theta)
    step = 1e-6
    assert lp.min() > 1e3 * step
    dx, dth = Pn.pnn_bwd64(x, theta, r)
    tx = torch.tensor(x, requires_grad=True)
    tt = torch.tensor(theta, requires_grad=True)
    tl = torch.sqrt((torch.einsum("if,bfe->bie", tt, tx) ** 2).sum(2))
    np.testing.assert_allclose(tl.detach().numpy(), lp, rtol=1e-13)
    (tl * torch.tensor(r)).sum().backward()
    np.testing.assert_allclose(dx, tx.grad.numpy(), rtol=1e-10, atol=1e-13)
    np.testing.assert_allclose(dth, tt.grad.numpy(), rtol=1e-10, atol=1e-13)
    f = lambda xx, th: float((r * Pn.pnn_fwd64(xx, th)[0]).sum())
    for k, v, got in (("x", x, dx), ("theta", theta, dth)):
        want = np.zeros(v.size)
        for i in range(v.size):
            hi, lo = v.copy(), v.copy()
            hi.reshape(-1)[i] += step
            lo.reshape(-1)[i] -= step
            want[i] = ((f(hi, theta) - f(lo, theta)) if k == "x" else (f(x, hi) - f(x, lo))) / (2 * step)
        want = want.reshape(v.shape)
        np.testing.assert_allclose(got, want, rtol=1e-6, atol=1e-7 * max(np.abs(want).max(), 1e-3), err_msg=k)


def test_an_all_padding_sample_has_zero_norm_and_zero_gradients():
    """lp = 0 exactly and finite, zero gradients from that sample (TF's tf.norm gives NaN there), in
    the formulas and in the autograd restatement."""
    x, theta, r = _point(5, 8, 6, 7)
    x[2] = 0.0
    lp, _ = Pn.pnn_fwd64(x, theta)
    assert (lp[2] == 0).all() and lp[[0, 1, 3]].min() > 0
    dx, dth = Pn.pnn_bwd64(x, theta, r)
    assert np.isfinite(dx).all() and np.isfinite(dth).all() and (dx[2] == 0).all()
    keep = [0, 1, 3]
    _, dth_keep = Pn.pnn_bwd64(x[keep], theta, r[keep])
    np.testing.assert_allclose(dth, dth_keep, rtol=1e-13, atol=0)
    # the restatement: a batch whose every id is the padding row 0
    name, kw = "dnn_cate", KW["dnn_cate"]
    cfg = R.make_cfg(name, **kw)
    P = Pn.init_params(cfg, 0, 0, True, np.random.default_rng(4), scale=0.3)
    b = Pn.X.make_batch(name, kw, 9, 2)
    b["cate_feats"] = np.asarray(b["cate_feats"]).copy()
    b["cate_feats"][4] = 0
    fw = Pn.forward_backward(cfg, P, b, pnn=True)
    assert (fw["lp"][4] == 0).all() and fw["lp"][[0, 1, 2, 3, 5]].min() > 0
    assert all(np.isfinite(g).all() for g in fw["G"].values()) and np.abs(fw["G"][Pn.KEY]).max() > 0


def test_restatement_gradients_match_the_formulas():
    """The autograd model's theta gradient equals pnn_bwd64 fed its own fields and ReluGrad-masked
    layer-0 gradient; the layer changes the logits and leaves the regulariser alone; with the cross
    network and the attention beside it as well."""
    name = "dnn_multi"
    kw = KW[name]
    cfg = R.make_cfg(name, **kw)
    for L, A in ((0, 0), (2, 3)):
        P = Pn.init_params(cfg, L, A, True, np.random.default_rng(8), scale=0.3)
        b = Pn.X.make_batch(name, kw, 23, 9)
        fw = Pn.forward_backward(cfg, P, b, L, A, True)
        # d = dL/dpre0 through the bias gradient's definition: recover it per sample by autograd-free algebra
        t = lambda a: torch.tensor(np.asarray(a, np.float64))
        pre0 = t(fw["pre0"]).requires_grad_(True)
        h = torch.relu(pre0)
        for i in range(1, len(cfg.hidden)):
            h = torch.relu(h @ t(P["deep_%d" % i]) + t(P["deep_bias_%d" % i]))
        zt = (h @ t(P["deep_res"]))[:, 0]
        y = b["label"].reshape(-1).astype(np.float64)
        p, eps = fw["p"], cfg.logloss_eps
        dz = (-y / (p + eps) + (1 - y) / (1 - p + eps)) / y.size * p * (1 - p)
        (zt * t(dz)).sum().backward()
        d = pre0.grad.numpy()
        np.testing.assert_allclose(fw["G"]["deep_bias_0"].reshape(-1), d.sum(0), rtol=1e-9, atol=1e-15)
        _, dth = Pn.pnn_bwd64(fw["fields"], P[Pn.KEY], d)
        np.testing.assert_allclose(fw["G"][Pn.KEY], dth, rtol=1e-9, atol=1e-15)
        plain = Pn.forward_backward(cfg, {k: v for k, v in P.items() if k != Pn.KEY}, b, L, A, False)
        assert np.abs(plain["z"] - fw["z"]).max() > 1e-6
        assert abs((fw["loss"] - fw["data"]) - (plain["loss"] - plain["data"])) < 1e-15


def test_model_spec_accepts_the_dnn_models():
    from deep_learning_amd.engine import ModelSpec
    assert ModelSpec("dnn_pipeline").pnn is None and ModelSpec("deepfm_pipeline").pnn is None
    for name, kw in KW.items():
        sp = ModelSpec(name, pnn="inner", **kw)
        assert sp.pnn == "inner" and sp.afm_fields == kw["S"] + len(kw.get("multi_ranges", []))
    sp = ModelSpec("dnn_cate", pnn="inner", afm_attention=4, cross_layers=2, dropout_keep_deep=[1, 1, 0.7],
                   pos_weight=2.0, **KW["dnn_cate"])
    assert sp.pnn == "inner" and sp.cross_layers == 2 and sp.dropout == [1.0, 1.0, 0.7]
    assert ModelSpec("dnn_pipeline", **dict(KW["dnn_pipeline"], pnn="inner", S=64, E=32)).afm_fields == 64


@pytest.mark.parametrize("model", ["deepfm_pipeline", "deepfm_cate", "deepfm_multi_cate", "deepfm_multi", "wdl",
                                   "dnn", "deepfm"])
def test_model_spec_refuses_other_models(model):
    from deep_learning_amd.engine import ModelSpec
    with pytest.raises(ValueError, match="pnn: the product layer feeds the tower of"):
        ModelSpec(model, pnn="inner")
    assert ModelSpec(model, pnn=None).pnn is None


def test_model_spec_refuses_what_the_layer_cannot_take():
    from deep_learning_amd.engine import ModelSpec
    kw = KW["dnn_pipeline"]
    with pytest.raises(ValueError, match="pnn: not supported with tower='bf16'"):
        ModelSpec("dnn_pipeline", pnn="inner", tower="bf16", **kw)
    with pytest.raises(ValueError, match="pnn: not supported with tower-input dropout"):
        ModelSpec("dnn_pipeline", pnn="inner", dropout_keep_deep=[0.9, 1, 1], **kw)
    with pytest.raises(ValueError, match=r"pnn: not supported with dropout on the first layer's output"):
        ModelSpec("dnn_pipeline", pnn="inner", dropout_keep_deep=[1, 0.9, 1], **kw)
    with pytest.raises(ValueError, match="pnn='outer'.*not built"):
        ModelSpec("dnn_pipeline", pnn="outer", **kw)
    for bad in ("Inner", "yes", 1, True, ""):
        with pytest.raises(ValueError, match="pnn must be None or 'inner'"):
            ModelSpec("dnn_pipeline", pnn=bad, **kw)
    for over in (dict(S=1), dict(S=65), dict(E=12), dict(E=64), dict(E=4)):
        with pytest.raises(ValueError, match="pnn: 2 to 64 embedded fields of size 8 / 16 / 32"):
            ModelSpec("dnn_pipeline", **dict(kw, pnn="inner", **over))
    with pytest.raises(ValueError, match="pnn"):       # 63 singles + 2 pooled = 65 fields
        ModelSpec("dnn_multi", **dict(KW["dnn_multi"], pnn="inner", S=63))


def test_sharded_engine_refuses():
    """Before anything touches a device or the exchange."""
    from deep_learning_amd.engine import ModelSpec
    from deep_learning_amd.shard import ShardedCTREngine
    ex = types.SimpleNamespace(world=1, rank=0)
    with pytest.raises(ValueError, match="pnn: not supported by ShardedCTREngine"):
        ShardedCTREngine(ModelSpec("dnn_pipeline", pnn="inner", **KW["dnn_pipeline"]), 64, ex)


def _argv(tmp_path, alg, *over):
    conf = tmp_path / "conf"
    if not conf.exists():
        conf.mkdir()
        lines = ["f%d\tx\tfloat" % i for i in range(13)] + ["c%d\tx\tstring" % i for i in range(26)]
        (conf / "dnn.conf").write_text("\n".join(lines) + "\n")
    return ["local_run.py", alg, "train", "1", "8", "3000", "3", str(conf), "tr/", "pr/", "pb", "ck", "0", "ck",
            "batch_size=64"] + list(over)


def test_local_run_override(tmp_path):
    """pnn=inner is parsed when given, absent from ModelParams.__dict__ (the start-up dump) when not,
    and reaches ModelSpec through _spec_from_args."""
    from deep_learning_amd.local_run import ModelParams
    from deep_learning_amd.models._ctr_model import _spec_from_args
    plain = ModelParams(_argv(tmp_path, "dnn_pipeline"))
    assert "pnn" not in plain.__dict__
    mp = ModelParams(_argv(tmp_path, "dnn_pipeline", "pnn=inner"))
    assert mp.pnn == "inner"
    assert set(mp.__dict__) - set(plain.__dict__) == {"pnn"}
    assert {k: v for k, v in mp.__dict__.items() if k in plain.__dict__} == plain.__dict__
    assert _spec_from_args("dnn_pipeline", mp).pnn == "inner"
    assert _spec_from_args("dnn_pipeline", plain).pnn is None


@pytest.mark.parametrize("alg,v,msg", [("dnn_pipeline", "outer", "not built"), ("dnn_pipeline", "1", "must be inner"),
                                       ("dnn_pipeline", "", "must be inner"),
                                       ("deepfm_pipeline", "inner", "feeds the tower")])
def test_local_run_refuses_bad_values(tmp_path, alg, v, msg):
    from deep_learning_amd.local_run import ModelParams
    with pytest.raises(SystemExit, match="pnn=.*" + msg):
        ModelParams(_argv(tmp_path, alg, "pnn=" + v))
