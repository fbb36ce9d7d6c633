"""CPU checks of AutoInt's interacting layers (ModelSpec.autoint_layers): the float64 closed forms of
tests/_autoint_ref.py against torch autograd, central differences and a case worked by hand; the model
restatement with the branch off and on; the parameter vector's pack / unpack; every refusal of ModelSpec,
ShardedCTREngine and local_run; the kernel fixture's acceptance at every GPU shape."""
import types

import numpy as np
import pytest

from oracle import ctr_ref as R
from tests import _autoint_ref as Ai
from tests import _cin_ref as Ci

KW = {"dnn_pipeline": dict(C=13, V=3, S=8, E=8, cate_index_size=1000, hidden=[16, 16]),
      "dnn_cate": dict(V=2, S=8, E=8, cate_index_size=1000, hidden=[16, 16]),
      "dnn_multi": dict(C=5, V=2, S=4, E=8, cate_index_size=1000, hidden=[16, 16],
                        multi_ranges=[[0, 7, "a"], [7, 12, "b"]]),
      "dnn_multi_cate": dict(V=0, S=4, E=8, cate_index_size=1000, hidden=[16, 16],
                             multi_ranges=[[0, 5, "a"], [5, 6, "b"]])}
AI = (2, 2, 8)


# --------------------------------------------------------------------------- the closed forms
@pytest.mark.parametrize("F,E,Hn,D,L", Ai.SHAPES[:5])
def test_closed_form_matches_torch_autograd(F, E, Hn, D, L):
    x, P, dz = Ai.kernel_fixture(7, F, E, Hn, D, L, F + L)
    z, _, _ = Ai.autoint_fwd64(x, P, L, Hn, D)
    dx, G = Ai.autoint_bwd64(x, P, L, Hn, D, dz)
    zt, dxt, Gt = Ai.torch_fwd_bwd(x, P, L, Hn, D, dz)
    np.testing.assert_allclose(z, zt, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(dx, dxt, rtol=1e-12, atol=1e-12 * np.abs(dxt).max())
    for k in Ai.keys(L):
        assert np.abs(Gt[k]).max() > 0, k
        np.testing.assert_allclose(G[k], Gt[k], rtol=1e-12, atol=1e-12 * np.abs(Gt[k]).max(), err_msg=k)


def test_closed_form_matches_central_differences():
    """d (sum_b dz z) by central differences in x and in every variable; the smallest |U| is far above the
    step, so no ReLU decision changes inside a difference."""
    F, E, Hn, D, L, h = 3, 8, 2, 8, 2, 1e-6
    x, P, dz = Ai.kernel_fixture(4, F, E, Hn, D, L, 5)
    x = x.astype(np.float64)
    P = {k: v.astype(np.float64) for k, v in P.items()}
    dz = dz.astype(np.float64)
    lo, _ = Ai.u_range(Ai.autoint_fwd64(x, P, L, Hn, D)[2])
    assert lo.min() > 100 * h
    dx, G = Ai.autoint_bwd64(x, P, L, Hn, D, dz)
    f = lambda xx, PP: float((Ai.autoint_fwd64(xx, PP, L, Hn, D)[0] * dz).sum())
    rng = np.random.default_rng(0)
    for _ in range(12):
        i = tuple(rng.integers(0, s) for s in x.shape)
        xp, xm = x.copy(), x.copy()
        xp[i] += h
        xm[i] -= h
        assert abs((f(xp, P) - f(xm, P)) / (2 * h) - dx[i]) < 1e-8 * max(1.0, np.abs(dx).max())
    for k in Ai.keys(L):
        for _ in range(4):
            i = tuple(rng.integers(0, s) for s in P[k].shape)
            Pp, Pm = dict(P), dict(P)
            Pp[k], Pm[k] = P[k].copy(), P[k].copy()
            Pp[k][i] += h
            Pm[k][i] -= h
            assert abs((f(x, Pp) - f(x, Pm)) / (2 * h) - G[k][i]) < 1e-8 * max(1.0, np.abs(G[k]).max()), k


def test_smallest_case_by_hand():
    """F = 2, Hn = 1, L = 1, written out without any array routine."""
    F, E, D = 2, 8, 8
    rng = np.random.default_rng(1)
    x = rng.standard_normal((1, F, E))
    P = {k: rng.standard_normal(s) * 0.4 for k, s in Ai.shapes(F, E, 1, D).items()}
    dot = lambda a, b: sum(float(p) * float(q) for p, q in zip(a, b))
    row = lambda v, W: [dot(v, W[:, c]) for c in range(D)]
    Q, K, V, Rr = ([row(x[0, f], P["autoint_%s_0" % m]) for f in range(F)] for m in "qkvr")
    z = 0.0
    for i in range(F):
        s = [dot(Q[i], K[k]) for k in range(F)]
        e = [np.exp(v) for v in s]
        a = [v / sum(e) for v in e]
        for c in range(D):
            u = sum(a[k] * V[k][c] for k in range(F)) + Rr[i][c]
            z += float(P["autoint_res"][i * D + c, 0]) * max(u, 0.0)
    got, _, _ = Ai.autoint_fwd64(x, P, 1, 1, D)
    assert abs(got[0] - z) < 1e-13 * max(1.0, abs(z))


def test_max_subtracted_softmax_is_the_bare_one():
    F, E, Hn, D, L = 5, 16, 4, 8, 2
    x, P, _ = Ai.kernel_fixture(6, F, E, Hn, D, L, 2)
    a, b = Ai.autoint_fwd64(x, P, L, Hn, D)[0], Ai.autoint_fwd64(x, P, L, Hn, D, stable=False)[0]
    np.testing.assert_allclose(a, b, rtol=1e-13, atol=1e-15)


def test_an_all_zero_sample_gives_nothing():
    F, E, Hn, D, L = 5, 16, 4, 8, 2
    x, P, dz = Ai.kernel_fixture(6, F, E, Hn, D, L, 2)
    x = x.copy()
    x[3] = 0
    z, _, _ = Ai.autoint_fwd64(x, P, L, Hn, D)
    dx, G = Ai.autoint_bwd64(x, P, L, Hn, D, dz)
    assert z[3] == 0 and not dx[3].any()
    keep = np.arange(6) != 3
    _, G2 = Ai.autoint_bwd64(x[keep], P, L, Hn, D, dz[keep])
    for k in G:
        np.testing.assert_allclose(G[k], G2[k], rtol=1e-13, atol=1e-18)


@pytest.mark.parametrize("name", list(KW))
def test_model_restatement(name):
    """autoint_layers = 0: oracle.ctr_ref's float64 forward and tests/_cin_ref.py's path exactly.  With the
    branch: its gradients are the closed forms fed the model's own fields and dz plus l2 w on autoint_res,
    l2 / 2 sum autoint_res^2 joins the loss, and it combines with the other branches."""
    kw = KW[name]
    cfg = R.make_cfg(name, **kw)
    b = Ai.X.make_batch(name, kw, 23, 9)
    P = R.init_params(cfg, np.random.default_rng(3))
    for off in (None, (0, 4, 32)):
        got = Ai.forward_backward(cfg, P, b, off)
        fw = R.forward(cfg, P, b, dtype=np.float64)
        np.testing.assert_allclose(got["z"], fw["z"], rtol=1e-12, atol=1e-14)
        assert abs(got["loss"] - fw["loss"]) < 1e-13
    P = Ci.init_params(cfg, np.random.default_rng(8), (4, 3), (2, 2), L=2, A=3)
    got, want = Ai.forward_backward(cfg, P, b, None, (4, 3), (2, 2), L=2, A=3), Ci.forward_backward(cfg, P, b, (4, 3), (2, 2), L=2, A=3)
    assert np.array_equal(got["z"], want["z"]) and got["loss"] == want["loss"]
    for k in P:
        assert np.array_equal(got["G"][k], want["G"][k]), k
    P = Ai.init_params(cfg, np.random.default_rng(8), AI, (4, 3), (2, 2), L=2, A=3)
    P["feats_emb"] = (P["feats_emb"] * 30).astype(np.float32)
    assert set(Ai.keys(AI[0])) <= set(P)
    fw = Ai.forward_backward(cfg, P, b, AI, (4, 3), (2, 2), L=2, A=3)
    assert 0 < fw["u_min"] < fw["u_max"]
    y = b["label"].reshape(-1).astype(np.float64)
    p, eps = fw["p"], cfg.logloss_eps
    dz = (-y / (p + eps) + (1 - y) / (1 - p + eps)) / y.size * p * (1 - p)
    L, Hn, D = AI
    _, G = Ai.autoint_bwd64(fw["fields"], P, L, Hn, D, dz)
    G["autoint_res"] = G["autoint_res"] + cfg.l2 * P["autoint_res"].astype(np.float64)
    for k in Ai.keys(L):
        assert np.abs(G[k]).max() > 0, k
        np.testing.assert_allclose(fw["G"][k].reshape(-1), G[k].reshape(-1), rtol=1e-9, atol=1e-15, err_msg=k)
    plain = Ci.forward_backward(cfg, {k: v for k, v in P.items() if not k.startswith("autoint_")}, b, (4, 3), (2, 2),
                                L=2, A=3)
    za, _, _ = Ai.autoint_fwd64(fw["fields"], P, L, Hn, D)
    np.testing.assert_allclose(fw["z"] - plain["z"], za, rtol=1e-9, atol=1e-13)
    assert np.abs(za).max() > 1e-3
    extra = (fw["loss"] - fw["data"]) - (plain["loss"] - plain["data"])
    assert abs(extra - cfg.l2 * 0.5 * float((P["autoint_res"].astype(np.float64) ** 2).sum())) < 1e-15


@pytest.mark.parametrize("F,E,Hn,D,L", Ai.SHAPES)
def test_fixture_accepts_enough_candidates(F, E, Hn, D, L):
    """The kernel fixture's condition at every GPU shape: B of 2 B candidates pass, every kept sample's
    smallest |U| is at least MARGIN times the largest, and no kept sample is dropped later."""
    B = 63
    x, P, dz, acc = Ai.kernel_fixture(B, F, E, Hn, D, L, 1000 * F + 10 * E + B, return_acceptance=True)
    assert x.shape == (B, F, E) and dz.shape == (B,) and acc >= 0.5
    lo, hi = Ai.u_range(Ai.autoint_fwd64(x, P, L, Hn, D)[2])
    assert lo.min() >= Ai.MARGIN * hi
    print("AUTOINT_FIXTURE F=%d E=%d Hn=%d D=%d L=%d acceptance %.2f" % (F, E, Hn, D, L, acc))


# --------------------------------------------------------------------------- the parameter vector
@pytest.mark.parametrize("F,E,Hn,D,L", Ai.SHAPES)
def test_pack_unpack_round_trip(F, E, Hn, D, L):
    """The engine's autoint_pack / autoint_unpack and the tests' own agree: [w | Wq_1 | Wk_1 | Wv_1 | Wr_1 |
    Wq_2 ..] row-major, bit for bit both ways; a variable of another size is refused."""
    from deep_learning_amd.param_groups import autoint_pack, autoint_shapes, autoint_unpack
    sh = autoint_shapes(F, E, L, D)
    assert sh == Ai.shapes(F, E, L, D) and list(sh) == Ai.keys(L)
    assert sh["autoint_res"] == (F * D, 1) and sh["autoint_q_0"] == (E, D) and sh["autoint_r_%d" % (L - 1)][1] == D
    if L > 1:
        assert sh["autoint_k_1"] == (D, D)
    P = Ai.init(F, E, L, D, np.random.default_rng(F))
    v = autoint_pack(P, sh)
    n = Ai.n_params(F, E, L, D)
    assert v.dtype == np.float32 and v.shape == (n,) and np.array_equal(v, Ai.pack(P, F, E, L, D))
    assert np.array_equal(v[:F * D], P["autoint_res"][:, 0])
    assert v[F * D + 1 * D + 2] == P["autoint_q_0"][1, 2] and v[F * D + E * D + 3] == P["autoint_k_0"][0, 3]
    assert v[F * D + 3 * E * D + 2 * D + 1] == P["autoint_r_0"][2, 1]
    back = autoint_unpack(v, sh)
    for k in P:
        assert back[k].shape == P[k].shape and np.array_equal(back[k], P[k]), k
    bad = dict(P, autoint_res=np.zeros(F * D + 1, np.float32))
    with pytest.raises(ValueError, match="autoint_layers: autoint_res holds"):
        autoint_pack(bad, sh)


# --------------------------------------------------------------------------- ModelSpec
def test_model_spec_accepts_the_dnn_models():
    from deep_learning_amd.engine import ModelSpec
    sp = ModelSpec("dnn_pipeline")
    assert (sp.autoint_layers, sp.autoint_heads, sp.autoint_dim) == (0, 2, 16)
    assert ModelSpec("deepfm_pipeline", autoint_heads=3, autoint_dim=5).autoint_layers == 0     # off, whatever they say
    for name, kw in KW.items():
        sp = ModelSpec(name, autoint_layers=2, autoint_heads=2, autoint_dim=8, **kw)
        assert (sp.autoint_layers, sp.autoint_heads, sp.autoint_dim) == (2, 2, 8)
    sp = ModelSpec("dnn_cate", autoint_layers=3, autoint_heads=4, autoint_dim=32, afm_attention=4, batch_norm=True,
                   bi_interaction=True, ccpm_filters=(2,), cin_layers=(4,), pos_weight=2.0,
                   **dict(KW["dnn_cate"], S=64, E=32))
    assert sp.afm_fields == 64 and sp.autoint_layers == 3
    assert ModelSpec("dnn_cate", autoint_layers=1, pnn="inner", dropout_keep_deep=[1, 1, 0.7], **KW["dnn_cate"]).pnn
    assert ModelSpec("dnn_cate", autoint_layers=1, autoint_heads=4, autoint_dim=8, **KW["dnn_cate"]).autoint_heads == 4


@pytest.mark.parametrize("model", ["deepfm_pipeline", "deepfm_cate", "deepfm_multi_cate", "deepfm_multi", "wdl",
                                   "dnn", "deepfm"])
def test_model_spec_refuses_other_models(model):
    from deep_learning_amd.engine import ModelSpec
    with pytest.raises(ValueError, match="autoint_layers.*join the tower"):
        ModelSpec(model, autoint_layers=1)
    assert ModelSpec(model, autoint_layers=0).autoint_layers == 0


def test_model_spec_refuses_what_the_branch_cannot_take():
    from deep_learning_amd.engine import ModelSpec
    kw = KW["dnn_pipeline"]
    with pytest.raises(ValueError, match="autoint_layers.*bf16"):
        ModelSpec("dnn_pipeline", autoint_layers=1, tower="bf16", **kw)
    with pytest.raises(ValueError, match="autoint_layers.*tower-input dropout"):
        ModelSpec("dnn_pipeline", autoint_layers=1, dropout_keep_deep=[0.9, 1, 1], **kw)
    for bad in (dict(autoint_layers="2"), dict(autoint_layers=1.5), dict(autoint_layers=1, autoint_heads=None),
                dict(autoint_layers=1, autoint_dim=(8,)), dict(autoint_layers=True)):
        with pytest.raises(ValueError, match="autoint_layers: autoint_\\w+ must be an integer"):
            ModelSpec("dnn_pipeline", **dict(kw, **bad))
    limits = [dict(autoint_layers=4), dict(autoint_layers=-1), dict(autoint_layers=1, autoint_heads=3),
              dict(autoint_layers=1, autoint_heads=8), dict(autoint_layers=1, autoint_heads=0),
              dict(autoint_layers=1, autoint_dim=12), dict(autoint_layers=1, autoint_dim=64),
              dict(autoint_layers=1, autoint_dim=4), dict(autoint_layers=1, autoint_heads=4, autoint_dim=4),
              dict(autoint_layers=1, E=12), dict(autoint_layers=1, E=4), dict(autoint_layers=1, E=64),
              dict(autoint_layers=1, S=1), dict(autoint_layers=1, S=65)]
    for over in limits:
        with pytest.raises(ValueError, match="autoint_layers: 1 to 3 layers of autoint_heads in 1 / 2 / 4 on "
                                             "autoint_dim in 8 / 16 / 32 columns with at least 2 a head, on 2 to 64"):
            ModelSpec("dnn_pipeline", **dict(kw, **over))
    with pytest.raises(ValueError, match="autoint_layers"):       # 63 singles + 2 pooled = 65 fields
        ModelSpec("dnn_multi", **dict(KW["dnn_multi"], autoint_layers=1, S=63))


def test_sharded_engine_refuses():
    """Before anything touches a device or the exchange."""
    from deep_learning_amd.engine import ModelSpec
    from deep_learning_amd.shard import ShardedCTREngine
    ex = types.SimpleNamespace(world=1, rank=0)
    with pytest.raises(ValueError, match="autoint_layers.*ShardedCTREngine"):
        ShardedCTREngine(ModelSpec("dnn_pipeline", autoint_layers=1, **KW["dnn_pipeline"]), 64, ex)


# --------------------------------------------------------------------------- local_run
def _argv(tmp_path, alg, *over, E="8", fields=26):
    conf = tmp_path / ("conf%d" % fields)
    if not conf.exists():
        conf.mkdir()
        lines = ["f%d\tx\tfloat" % i for i in range(13)] + ["c%d\tx\tstring" % i for i in range(fields)]
        (conf / "dnn.conf").write_text("\n".join(lines) + "\n")
    return ["local_run.py", alg, "train", "1", E, "3000", "3", str(conf), "tr/", "pr/", "pb", "ck", "0", "ck",
            "batch_size=64"] + list(over)


def test_local_run_override(tmp_path):
    """The three overrides are parsed when given, absent from ModelParams.__dict__ (the start-up dump) when
    not, and reach ModelSpec through _spec_from_args."""
    from deep_learning_amd.local_run import ModelParams
    from deep_learning_amd.models._ctr_model import _spec_from_args
    plain = ModelParams(_argv(tmp_path, "dnn_pipeline"))
    assert not any(k.startswith("autoint") for k in plain.__dict__)
    mp = ModelParams(_argv(tmp_path, "dnn_pipeline", "autoint_layers=2", "autoint_heads=4", "autoint_dim=32"))
    assert (mp.autoint_layers, mp.autoint_heads, mp.autoint_dim) == (2, 4, 32)
    sp = _spec_from_args("dnn_pipeline", mp)
    assert (sp.autoint_layers, sp.autoint_heads, sp.autoint_dim) == (2, 4, 32)
    mp = ModelParams(_argv(tmp_path, "dnn_cate", "autoint_layers=1"))
    assert mp.autoint_layers == 1 and not hasattr(mp, "autoint_heads")
    sp = _spec_from_args("dnn_cate", mp)
    assert (sp.autoint_layers, sp.autoint_heads, sp.autoint_dim) == (1, 2, 16)
    assert ModelParams(_argv(tmp_path, "deepfm_pipeline", "autoint_layers=0", "autoint_heads=3")).autoint_layers == 0
    assert _spec_from_args("dnn_pipeline", plain).autoint_layers == 0


@pytest.mark.parametrize("alg,over,msg", [
    ("dnn_pipeline", ["autoint_layers=two"], "autoint_layers: autoint_layers=two is not an integer"),
    ("dnn_pipeline", ["autoint_layers=1", "autoint_dim=1.5"], "autoint_layers: autoint_dim=1.5 is not an integer"),
    ("deepfm_pipeline", ["autoint_layers=1"], "autoint_layers=1: the interacting layers join the tower of"),
    ("dnn_pipeline", ["autoint_layers=4"], "autoint_layers: 1 to 3 layers"),
    ("dnn_pipeline", ["autoint_layers=1", "autoint_heads=3"], "autoint_layers: 1 to 3 layers"),
    ("dnn_pipeline", ["autoint_layers=1", "autoint_dim=12"], "autoint_layers: 1 to 3 layers"),
    ("dnn_pipeline", ["autoint_heads=4", "autoint_dim=4", "autoint_layers=2"], "autoint_layers: 1 to 3 layers")])
def test_local_run_refuses_bad_values(tmp_path, alg, over, msg):
    from deep_learning_amd.local_run import ModelParams
    with pytest.raises(SystemExit, match=msg):
        ModelParams(_argv(tmp_path, alg, *over))


@pytest.mark.parametrize("E,fields", [("12", 26), ("8", 1), ("8", 65), ("64", 26)])
def test_local_run_refuses_fields_outside_the_limits(tmp_path, E, fields):
    from deep_learning_amd.local_run import ModelParams
    with pytest.raises(SystemExit, match="autoint_layers: 1 to 3 layers.*got autoint_layers=1"):
        ModelParams(_argv(tmp_path, "dnn_pipeline", "autoint_layers=1", E=E, fields=fields))
    ModelParams(_argv(tmp_path, "dnn_pipeline", E=E, fields=fields))      # without the override nothing is refused
