"""CPU checks of the attentional pairwise interactions (ModelSpec.afm_attention): the
float64 restatement (tests/_afm_ref.py) pinned to the oracle at afm_attention = 0, the backward
formulas against autograd and finite differences, the F = 2 and softmax identities, the dyadic
kernel fixture's exactness, ModelSpec's refusals and local_run's afm_attention= override."""
import types

import numpy as np
import pytest
import torch

from oracle import ctr_ref as R
from tests import _afm_ref as Af

KW = {"dnn_pipeline": dict(C=5, V=3, S=6, E=8, cate_index_size=300, hidden=[16, 8]),
      "dnn_cate": dict(V=2, S=6, E=8, cate_index_size=300, hidden=[16, 8]),
      "dnn_multi": dict(C=5, V=2, S=4, E=8, cate_index_size=300, hidden=[16, 8],
                        multi_ranges=[[0, 7, "a"], [7, 12, "b"]]),
      "dnn_multi_cate": dict(V=0, S=4, E=8, cate_index_size=300, hidden=[16, 8],
                             multi_ranges=[[0, 5, "a"], [5, 6, "b"]])}


@pytest.mark.parametrize("name", list(KW))
def test_restatement_is_the_oracle_without_the_branch(name):
    """afm_attention = 0: logits, loss and every parameter gradient equal ctr_ref.forward /
    ctr_ref.backward run in float64, to float64 rounding."""
    kw = KW[name]
    cfg = R.make_cfg(name, **kw)
    P = Af.init_params(cfg, 0, 0, np.random.default_rng(3))
    assert set(P) == set(R.init_params(cfg, np.random.default_rng(3)))
    b = Af.X.make_batch(name, kw, 37, 5)
    got = Af.forward_backward(cfg, P, b, 0, 0)
    fw = R.forward(cfg, P, b, dtype=np.float64)
    G, _ = R.backward(cfg, P, b, fw, dtype=np.float64)
    np.testing.assert_allclose(got["z"], fw["z"], rtol=1e-12, atol=1e-14)
    assert abs(got["loss"] - fw["loss"]) < 1e-13
    for k in P:
        scale = np.abs(G[k]).max()
        assert scale > 0, k
        np.testing.assert_allclose(got["G"][k], G[k], rtol=0, atol=1e-12 * scale, err_msg=k)


def _point(F, E, A, seed, B=4):
    rng = np.random.default_rng(seed)
    return dict(x=rng.standard_normal((B, F, E)), p=rng.standard_normal(E), h=rng.standard_normal(A),
                b=rng.standard_normal(A) * 0.5, W=rng.standard_normal((E, A)) * 0.5), rng.standard_normal(B)


@pytest.mark.parametrize("F,E,A", [(2, 8, 1), (3, 4, 5), (7, 8, 3)])
def test_backward_formulas_match_autograd_and_finite_differences(F, E, A):
    """afm_bwd64 against torch autograd of sum_b r_b z_afm_b (1e-10 relative) and against central
    differences with step 1e-6, at a point whose smallest |u| is asserted above the step's reach."""
    v, r = _point(F, E, A, 100 * F + A)
    z, _, _, q, u = Af.afm_fwd64(**v)
    step = 1e-6
    assert np.abs(u).min() > 1e3 * step          # no ReLU kink within the differences' reach
    dx, dp, dh, db, dW = Af.afm_bwd64(dz=r, **v)
    got = dict(x=dx, p=dp, h=dh, b=db, W=dW)
    # autograd
    T = {k: torch.tensor(a, dtype=torch.float64, requires_grad=True) for k, a in v.items()}
    pi, pj = Af.pairs(F)
    tq = T["x"][:, pi] * T["x"][:, pj]
    ts = (torch.relu(tq @ T["W"] + T["b"]) * T["h"]).sum(2)
    tz = ((torch.softmax(ts, 1)[:, :, None] * tq).sum(1) * T["p"]).sum(1)
    np.testing.assert_allclose(tz.detach().numpy(), z, rtol=1e-12, atol=1e-14)
    (tz * torch.tensor(r)).sum().backward()
    for k in v:
        np.testing.assert_allclose(got[k], T[k].grad.numpy(), rtol=1e-10, atol=1e-13, err_msg=k)
    # central differences
    f = lambda vv: float(r @ Af.afm_fwd64(**vv)[0])
    for k in v:
        want = np.zeros(v[k].size)
        for i in range(v[k].size):
            hi, lo = v[k].copy(), v[k].copy()
            hi.reshape(-1)[i] += step
            lo.reshape(-1)[i] -= step
            want[i] = (f(dict(v, **{k: hi})) - f(dict(v, **{k: lo}))) / (2 * step)
        want = want.reshape(v[k].shape)
        np.testing.assert_allclose(got[k], want, rtol=1e-6, atol=1e-7 * max(np.abs(want).max(), 1e-3), err_msg=k)


def test_two_fields_have_one_pair_of_weight_one():
    v, _ = _point(2, 8, 3, 5)
    z, stats, a, _, _ = Af.afm_fwd64(**v)
    assert a.shape == (4, 1) and (a == 1.0).all() and (stats[:, 1] == 1.0).all()
    assert np.array_equal(z, ((v["x"][:, 0] * v["x"][:, 1]) * v["p"]).sum(1))


def test_max_subtracted_softmax_is_the_bare_one():
    v, _ = _point(6, 8, 4, 9)
    _, stats, a, q, u = Af.afm_fwd64(**v)
    s = (np.maximum(u, 0) * v["h"]).sum(2)
    bare = np.exp(s) / np.exp(s).sum(1, keepdims=True)
    assert np.isfinite(bare).all()
    np.testing.assert_allclose(a, bare, rtol=1e-13, atol=0)
    np.testing.assert_array_equal(stats[:, 0], s.max(1))


def test_restatement_branch_gradients_match_the_formulas():
    """The autograd model's attention gradients equal the formulas fed its own fields and dz, and
    the branch leaves the regulariser alone; with the cross network beside it as well."""
    name, A = "dnn_multi", 3
    kw = KW[name]
    cfg = R.make_cfg(name, **kw)
    for L in (0, 2):
        P = Af.init_params(cfg, L, A, np.random.default_rng(8))
        assert set(Af.AFM_KEYS) <= set(P)
        b = Af.X.make_batch(name, kw, 23, 9)
        fw = Af.forward_backward(cfg, P, b, L, A)
        y = b["label"].reshape(-1).astype(np.float64)
        p, eps = fw["p"], cfg.logloss_eps
        dz = (-y / (p + eps) + (1 - y) / (1 - p + eps)) / y.size * p * (1 - p)
        F = kw["S"] + len(kw["multi_ranges"])
        x = fw["x0"][:, kw["C"] + kw["V"]:].reshape(23, F, kw["E"])
        _, dp, dh, db, dW = Af.afm_bwd64(x, P["attention_p"], P["attention_h"], P["attention_b"], P["attention_w"], dz)
        for k, g in (("attention_p", dp), ("attention_h", dh), ("attention_b", db), ("attention_w", dW)):
            np.testing.assert_allclose(fw["G"][k].reshape(-1), g.reshape(-1), rtol=1e-9, atol=1e-15, err_msg=k)
        plain = Af.forward_backward(cfg, {k: v for k, v in P.items() if k not in Af.AFM_KEYS}, b, L, 0)
        assert np.abs(plain["z"] - fw["z"]).max() > 1e-6
        assert abs((fw["loss"] - fw["data"]) - (plain["loss"] - plain["data"])) < 1e-15


@pytest.mark.parametrize("F,E,A", [(2, 8, 1), (3, 16, 5), (26, 16, 16), (33, 8, 32), (64, 32, 7)])
def test_dyadic_fixture_makes_u_exact(F, E, A):
    """Every u of the kernels' fixture is an odd multiple of 1/1024: evaluated in f32 and in f64 it
    has the same bits (also with the sum over e reversed), and min |u| >= 1/1024."""
    x, p, h, b, W, dz = Af.dyadic_fixture(5, F, E, A, seed=F + A)
    _, u64, _ = Af.afm_scores64(x, b, W, h, np.float64)
    _, u32, _ = Af.afm_scores64(x, b, W, h, np.float32)
    _, u32r, _ = Af.afm_scores64(x[:, :, ::-1], b, W[::-1], h, np.float32)
    assert u32.dtype == np.float32 and np.array_equal(u32.astype(np.float64), u64)
    assert np.array_equal(u32r, u32)
    assert np.abs(u64).min() >= 1.0 / 1024
    k = u64 * 1024
    assert np.array_equal(k, np.round(k)) and (np.abs(k) % 2 == 1).all()
    assert len(Af.pack(p, h, b, W)) % 4 == 0


def test_model_spec_accepts_the_dnn_models():
    from deep_learning_amd.engine import ModelSpec
    assert ModelSpec("dnn_pipeline").afm_attention == 0 and ModelSpec("deepfm_pipeline").afm_attention == 0
    assert ModelSpec.AFM_MAX_ATT == 32 and ModelSpec.AFM_MAX_FIELDS == 64
    for name, kw in KW.items():
        sp = ModelSpec(name, afm_attention=4, **kw)
        assert sp.afm_attention == 4 and sp.afm_fields == kw["S"] + len(kw.get("multi_ranges", []))
    sp = ModelSpec("dnn_cate", afm_attention=32, cross_layers=2, dropout_keep_deep=[1, 0.8, 0.7], pos_weight=2.0,
                   **KW["dnn_cate"])
    assert sp.afm_attention == 32 and sp.cross_layers == 2 and sp.dropout == [1.0, 0.8, 0.7]


@pytest.mark.parametrize("model", ["deepfm_pipeline", "deepfm_cate", "deepfm_multi_cate", "deepfm_multi", "wdl",
                                   "dnn", "deepfm"])
def test_model_spec_refuses_other_models(model):
    from deep_learning_amd.engine import ModelSpec
    with pytest.raises(ValueError, match="afm_attention.*join the tower"):
        ModelSpec(model, afm_attention=4)
    assert ModelSpec(model, afm_attention=0).afm_attention == 0


def test_model_spec_refuses_what_the_branch_cannot_take():
    from deep_learning_amd.engine import ModelSpec
    kw = KW["dnn_pipeline"]
    with pytest.raises(ValueError, match="afm_attention.*bf16"):
        ModelSpec("dnn_pipeline", afm_attention=4, tower="bf16", **kw)
    with pytest.raises(ValueError, match="afm_attention.*tower-input dropout"):
        ModelSpec("dnn_pipeline", afm_attention=4, dropout_keep_deep=[0.9, 1, 1], **kw)
    for bad in (-1, 1.5):
        with pytest.raises(ValueError, match="afm_attention must be an integer"):
            ModelSpec("dnn_pipeline", afm_attention=bad, **kw)
    for over in (dict(afm_attention=33), dict(afm_attention=4, S=1), dict(afm_attention=4, S=65),
                 dict(afm_attention=4, E=12), dict(afm_attention=4, E=64)):
        with pytest.raises(ValueError, match="afm_attention: at most 32 attention units on 2 to 64"):
            ModelSpec("dnn_pipeline", **dict(kw, **over))
    assert ModelSpec("dnn_pipeline", **dict(kw, afm_attention=1, S=64, E=32)).afm_fields == 64
    with pytest.raises(ValueError, match="afm_attention"):       # 63 singles + 2 pooled = 65 fields
        ModelSpec("dnn_multi", **dict(KW["dnn_multi"], afm_attention=4, S=63))


def test_sharded_engine_refuses():
    """Before anything touches a device or the exchange."""
    from deep_learning_amd.engine import ModelSpec
    from deep_learning_amd.shard import ShardedCTREngine
    ex = types.SimpleNamespace(world=1, rank=0)
    with pytest.raises(ValueError, match="afm_attention.*ShardedCTREngine"):
        ShardedCTREngine(ModelSpec("dnn_pipeline", afm_attention=4, **KW["dnn_pipeline"]), 64, ex)


def _argv(tmp_path, alg, *over):
    conf = tmp_path / "conf"
    if not conf.exists():
        conf.mkdir()
        lines = ["f%d\tx\tfloat" % i for i in range(13)] + ["c%d\tx\tstring" % i for i in range(26)]
        (conf / "dnn.conf").write_text("\n".join(lines) + "\n")
    return ["local_run.py", alg, "train", "1", "8", "3000", "3", str(conf), "tr/", "pr/", "pb", "ck", "0", "ck",
            "batch_size=64"] + list(over)


def test_local_run_override(tmp_path):
    """afm_attention=A is parsed when given, absent from ModelParams.__dict__ (the start-up dump)
    when not, and reaches ModelSpec through _spec_from_args."""
    from deep_learning_amd.local_run import ModelParams
    from deep_learning_amd.models._ctr_model import _spec_from_args
    plain = ModelParams(_argv(tmp_path, "dnn_pipeline"))
    assert "afm_attention" not in plain.__dict__
    mp = ModelParams(_argv(tmp_path, "dnn_pipeline", "afm_attention=16"))
    assert mp.afm_attention == 16
    assert set(mp.__dict__) - set(plain.__dict__) == {"afm_attention"}
    assert {k: v for k, v in mp.__dict__.items() if k in plain.__dict__} == plain.__dict__
    assert _spec_from_args("dnn_pipeline", mp).afm_attention == 16
    assert _spec_from_args("dnn_pipeline", plain).afm_attention == 0
    assert ModelParams(_argv(tmp_path, "deepfm_pipeline", "afm_attention=0")).afm_attention == 0


@pytest.mark.parametrize("alg,v,msg", [("dnn_pipeline", "-1", "must lie in"), ("dnn_pipeline", "abc", "not an integer"),
                                       ("dnn_pipeline", "1.5", "not an integer"), ("dnn_pipeline", "33", "must lie in"),
                                       ("dnn_pipeline", "", "not an integer"),
                                       ("deepfm_pipeline", "2", "join the tower")])
def test_local_run_refuses_bad_values(tmp_path, alg, v, msg):
    from deep_learning_amd.local_run import ModelParams
    with pytest.raises(SystemExit, match="afm_attention=.*" + msg):
        ModelParams(_argv(tmp_path, alg, "afm_attention=" + v))
