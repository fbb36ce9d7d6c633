"""CPU checks of the CCPM branch (ModelSpec.ccpm_filters): the numpy restatement
(tests/_ccpm_ref.py) against torch-CPU float64 autograd (F.conv2d(padding=1), relu, F.max_pool2d(2), a dot
product) to 1e-12, the crafted tie case among the points; the rounding margin measured again; the whole-model
restatement pinned to tests/_bi_ref.py without the branch and to the formulas with it; the parameter
vector's pack / unpack; every refusal of ModelSpec, ShardedCTREngine and local_run; the ccpm_filters=
override."""
import types

import numpy as np
import pytest

from oracle import ctr_ref as R
from tests import _bi_ref as Bi
from tests import _ccpm_ref as Cc

KW = {"dnn_pipeline": dict(C=5, V=3, S=6, E=8, cate_index_size=300, hidden=[16, 8]),
      "dnn_cate": dict(V=2, S=6, E=8, cate_index_size=300, hidden=[16, 8]),
      "dnn_multi": dict(C=5, V=2, S=4, E=8, cate_index_size=300, hidden=[16, 8],
                        multi_ranges=[[0, 7, "a"], [7, 12, "b"]]),
      "dnn_multi_cate": dict(V=0, S=4, E=8, cate_index_size=300, hidden=[16, 8],
                             multi_ranges=[[0, 5, "a"], [5, 6, "b"]])}


def _against_torch(x, P, filters, dz):
    z, _ = Cc.ccpm_fwd(x, P, filters)
    dx, G = Cc.ccpm_bwd(x, P, filters, dz)
    zt, dxt, Gt = Cc.torch_fwd_bwd(x, P, filters, dz)
    assert set(G) == set(Gt) == set(Cc.keys(filters))
    np.testing.assert_allclose(z, zt, rtol=1e-12, atol=1e-12 * np.abs(zt).max())
    assert np.abs(dxt).max() > 0
    np.testing.assert_allclose(dx, dxt, rtol=0, atol=1e-12 * np.abs(dxt).max())
    for k in G:
        assert G[k].shape == np.shape(P[k]) and np.abs(Gt[k]).max() > 0, k
        np.testing.assert_allclose(G[k], Gt[k].reshape(G[k].shape), rtol=0, atol=1e-12 * np.abs(Gt[k]).max(), err_msg=k)


@pytest.mark.parametrize("F,E,filters", Cc.SHAPES + [(5, 16, (3,)), (8, 8, (8, 8, 8))])
def test_restatement_matches_torch_autograd(F, E, filters):
    """Forward, dX and every parameter gradient within 1e-12 (relative to the largest value) of autograd,
    the kernels permuted to torch's [C_out, C_in, 3, 3]; B = 7 with an all-zero sample."""
    x, P, dz = Cc.kernel_fixture(7, F, E, filters, seed=F + E)
    _against_torch(x, P, filters, dz)


@pytest.mark.parametrize("F,E,filters", [(9, 8, (2, 3, 2)), (6, 8, (4,)), (26, 16, (4, 4))])
def test_crafted_ties_go_to_the_first_maximum(F, E, filters):
    """Constant and pairwise-repeated maps of dyadic values: windows whose positive maximum is attained
    two to four times, exactly; the restatement and torch's max_pool2d send the gradient to the same
    (first) position.  Every u is exact in float32 too."""
    x, P, dz = Cc.tie_fixture(12, F, E, filters, seed=5)
    assert Cc.positive_ties(x, P, filters) > 20
    _against_torch(x, P, filters, dz)
    _, t64 = Cc.ccpm_fwd(x, P, filters, np.float64)
    _, t32 = Cc.ccpm_fwd(x, P, filters, np.float32)
    for a, b in zip(t32, t64):
        assert a[1].dtype == np.float32 and np.array_equal(a[1].astype(np.float64), b[1])
        assert np.array_equal(a[3], b[3])


def test_odd_rows_and_columns_are_read_but_get_no_pool_gradient():
    """F = 3: the third column feeds the convolution at column 1 and is dropped by the pool; changing it
    changes z, and with a 1 x 1 kernel support (only the centre tap nonzero) it receives no gradient."""
    F, E, filters = 3, 8, (2,)
    x, P, dz = Cc.kernel_fixture(5, F, E, filters, seed=3)
    z0, _ = Cc.ccpm_fwd(x, P, filters)
    x2 = x.copy()
    x2[:, 2] += 0.5
    assert np.abs(Cc.ccpm_fwd(x2, P, filters)[0] - z0).max() > 1e-4
    Pc = {k: v.copy() for k, v in P.items()}
    K = np.zeros_like(Pc["ccpm_conv_0.kernel"])
    K[1, 1] = P["ccpm_conv_0.kernel"][1, 1]
    Pc["ccpm_conv_0.kernel"] = K
    dx, _ = Cc.ccpm_bwd(x, Pc, filters, dz)
    assert (dx[:, 2] == 0).all() and np.abs(dx[:, :2]).max() > 0


def test_rounding_margin():
    """The largest |u_32 - u_64| / max |u_l| over the GPU test's shapes stays within U32_REL, MARGIN is 8
    times it, and at that margin the restatement alone stays within the GPU test's caps."""
    assert Cc.MARGIN == 8 * Cc.U32_REL
    worst = 0.0
    for F, E, filters in Cc.SHAPES:
        B = 300 if F < 64 else 63
        x, P, _ = Cc.kernel_fixture(B, F, E, filters, seed=1000 * F + 10 * E + B)
        worst = max(worst, Cc.u_rel_error(x, P, filters))
        und = Cc.undecided(x, P, filters)
        assert und.mean() <= (0.5 if F == 64 else 0.1) and (~und).sum() >= 1, (F, E, filters, und.mean())
    print("largest relative |u32 - u64|: %.3g" % worst)
    assert 0 < worst <= Cc.U32_REL


def test_undecided_flags_small_signs_and_close_pairs():
    F, E, filters = 4, 8, (1,)
    P = {k: np.zeros(s, np.float32) for k, s in Cc.shapes(F, E, filters).items()}
    P["ccpm_conv_0.kernel"][1, 1, 0, 0] = 1.0          # u = x
    x = np.ones((3, F, E), np.float32) + np.arange(F * E, dtype=np.float32).reshape(F, E)[None] * 0.25
    assert not Cc.undecided(x, P, filters).any()
    x[1, 0, 0] = 1e-6                                  # a sign within the margin of max |u| ~ 9
    x[2, 1, 1] = x[2, 1, 0] + 1e-6                     # a positive window's two largest within it
    assert Cc.undecided(x, P, filters).tolist() == [False, True, True]
    x[2, 1, 1] = x[2, 1, 0] = x[2, 0, 1] = x[2, 0, 0] = 20.0
    assert Cc.undecided(x, P, filters)[2] and not Cc.undecided(x, P, filters, exact_ties_ok=True)[2]


@pytest.mark.parametrize("name", list(KW))
def test_model_restatement(name):
    """ccpm_filters = (): tests/_bi_ref.py's logits, loss and gradients exactly.  With the branch: its
    gradients are the formulas fed the model's own fields and dz, the regulariser is untouched, and it
    combines with the cross network and the attention."""
    kw = KW[name]
    cfg = R.make_cfg(name, **kw)
    b = Cc.X.make_batch(name, kw, 23, 9)
    P = Cc.init_params(cfg, np.random.default_rng(8), (), L=2, A=3)
    got, want = Cc.forward_backward(cfg, P, b, (), L=2, A=3), Bi.forward_backward(cfg, P, b, L=2, A=3)
    assert np.array_equal(got["z"], want["z"]) and got["loss"] == want["loss"]
    for k in P:
        assert np.array_equal(got["G"][k], want["G"][k]), k
    filters = (2, 2)
    P = Cc.init_params(cfg, np.random.default_rng(8), filters, L=2, A=3)
    P["feats_emb"] = (P["feats_emb"] * 30).astype(np.float32)
    assert set(Cc.keys(filters)) <= set(P)
    fw = Cc.forward_backward(cfg, P, b, filters, L=2, A=3)
    y = b["label"].reshape(-1).astype(np.float64)
    p, eps = fw["p"], cfg.logloss_eps
    dz = (-y / (p + eps) + (1 - y) / (1 - p + eps)) / y.size * p * (1 - p)
    _, G = Cc.ccpm_bwd(fw["fields"], P, filters, dz)
    for k in Cc.keys(filters):
        assert np.abs(G[k]).max() > 0, k
        np.testing.assert_allclose(fw["G"][k].reshape(-1), G[k].reshape(-1), rtol=1e-9, atol=1e-15, err_msg=k)
    plain = Cc.forward_backward(cfg, {k: v for k, v in P.items() if not k.startswith("ccpm_")}, b, (), L=2, A=3)
    zc, _ = Cc.ccpm_fwd(fw["fields"], P, filters)
    np.testing.assert_allclose(fw["z"] - plain["z"], zc, rtol=1e-9, atol=1e-13)
    assert np.abs(zc).max() > 1e-3
    assert abs((fw["loss"] - fw["data"]) - (plain["loss"] - plain["data"])) < 1e-15


# --------------------------------------------------------------------------- the parameter vector
@pytest.mark.parametrize("F,E,filters", Cc.SHAPES)
def test_pack_unpack_round_trip(F, E, filters):
    """The engine's ccpm_pack / ccpm_unpack and the tests' own agree: [p | K_0 | b_0 | K_1 | b_1 ..] in the
    reference's Keras shapes, bit for bit both ways; a variable of another size is refused."""
    from deep_learning_amd.engine import ModelSpec, ccpm_pack, ccpm_shapes, ccpm_unpack
    sp = ModelSpec("dnn_cate", S=F, E=E, ccpm_filters=filters)
    shapes = ccpm_shapes(sp.ccpm_dims())
    assert shapes == Cc.shapes(F, E, filters) and list(shapes) == Cc.keys(filters)
    H, W = E >> len(filters), F >> len(filters)
    assert shapes["ccpm_out.kernel"] == (H * W * filters[-1], 1)
    assert shapes["ccpm_conv_0.kernel"] == (3, 3, 1, filters[0])
    P = Cc.init(F, E, filters, np.random.default_rng(F), bias=0.1)
    v = ccpm_pack(P, shapes)
    n = Cc.n_params(F, E, filters)
    assert v.dtype == np.float32 and v.shape == (n,) and np.array_equal(v, Cc.pack(P, F, E, filters)[:n])
    o = shapes["ccpm_out.kernel"][0]
    assert np.array_equal(v[:o], P["ccpm_out.kernel"][:, 0])
    assert np.array_equal(v[o:o + 9 * filters[0]], P["ccpm_conv_0.kernel"].reshape(-1))
    back = ccpm_unpack(v, shapes)
    for k in P:
        assert back[k].shape == P[k].shape and np.array_equal(back[k], P[k]), k
    bad = dict(P, **{"ccpm_conv_0.bias": np.zeros(filters[0] + 1, np.float32)})
    with pytest.raises(ValueError, match="ccpm_filters: ccpm_conv_0.bias holds"):
        ccpm_pack(bad, shapes)


# --------------------------------------------------------------------------- ModelSpec
def test_model_spec_accepts_the_dnn_models():
    from deep_learning_amd.engine import ModelSpec
    assert ModelSpec("dnn_pipeline").ccpm_filters == () and ModelSpec("deepfm_pipeline").ccpm_filters == ()
    assert (ModelSpec.CCPM_MAX_LAYERS, ModelSpec.CCPM_MAX_FILTERS, ModelSpec.CCPM_MAX_FIELDS) == (3, 8, 64)
    for name, kw in KW.items():
        sp = ModelSpec(name, ccpm_filters=[2, 2], **kw)
        F = kw["S"] + len(kw.get("multi_ranges", []))
        assert sp.ccpm_filters == (2, 2) and sp.ccpm_dims() == [(8, F, 1), (4, F // 2, 2), (2, F // 4, 2)]
    sp = ModelSpec("dnn_cate", ccpm_filters=(8, 8, 8), afm_attention=4, batch_norm=True,
                   bi_interaction=True, pos_weight=2.0, **dict(KW["dnn_cate"], S=64, E=32))
    assert sp.ccpm_filters == (8, 8, 8) and sp.afm_fields == 64
    assert ModelSpec("dnn_cate", ccpm_filters=(1,), pnn="inner", dropout_keep_deep=[1, 1, 0.7], **KW["dnn_cate"]).pnn


@pytest.mark.parametrize("model", ["deepfm_pipeline", "deepfm_cate", "deepfm_multi_cate", "deepfm_multi", "wdl",
                                   "dnn", "deepfm"])
def test_model_spec_refuses_other_models(model):
    from deep_learning_amd.engine import ModelSpec
    with pytest.raises(ValueError, match="ccpm_filters.*join the tower"):
        ModelSpec(model, ccpm_filters=(2,))
    assert ModelSpec(model, ccpm_filters=()).ccpm_filters == ()


def test_model_spec_refuses_what_the_branch_cannot_take():
    from deep_learning_amd.engine import ModelSpec
    kw = KW["dnn_pipeline"]
    with pytest.raises(ValueError, match="ccpm_filters.*bf16"):
        ModelSpec("dnn_pipeline", ccpm_filters=(2,), tower="bf16", **kw)
    with pytest.raises(ValueError, match="ccpm_filters.*tower-input dropout"):
        ModelSpec("dnn_pipeline", ccpm_filters=(2,), dropout_keep_deep=[0.9, 1, 1], **kw)
    for bad in (4, "ab", (1.5,), (2, None)):
        with pytest.raises(ValueError, match="ccpm_filters must be a sequence of integers"):
            ModelSpec("dnn_pipeline", ccpm_filters=bad, **kw)
    limits = [dict(ccpm_filters=(2, 2, 2, 2), S=32, E=32),       # L = 4
              dict(ccpm_filters=(0,)), dict(ccpm_filters=(9,)), dict(ccpm_filters=(2, -1)),
              dict(ccpm_filters=(2,), E=12), dict(ccpm_filters=(2,), E=4), dict(ccpm_filters=(2,), E=64),
              dict(ccpm_filters=(2,), S=1), dict(ccpm_filters=(2,), S=65),
              dict(ccpm_filters=(2, 2), S=3),                    # 3 -> 1 -> 0 columns
              dict(ccpm_filters=(2, 2, 2), S=7)]
    for over in limits:
        with pytest.raises(ValueError, match="ccpm_filters: 1 to 3 layers of 1 to 8 filters on 2 to 64"):
            ModelSpec("dnn_pipeline", **dict(kw, **over))
    assert ModelSpec("dnn_pipeline", **dict(kw, ccpm_filters=(8, 8, 8), S=64, E=32)).afm_fields == 64
    assert ModelSpec("dnn_pipeline", **dict(kw, ccpm_filters=(1, 1, 1), S=8, E=8)).ccpm_dims()[-1] == (1, 1, 1)
    with pytest.raises(ValueError, match="ccpm_filters"):       # 63 singles + 2 pooled = 65 fields
        ModelSpec("dnn_multi", **dict(KW["dnn_multi"], ccpm_filters=(2,), S=63))


def test_sharded_engine_refuses():
    """Before anything touches a device or the exchange."""
    from deep_learning_amd.engine import ModelSpec
    from deep_learning_amd.shard import ShardedCTREngine
    ex = types.SimpleNamespace(world=1, rank=0)
    with pytest.raises(ValueError, match="ccpm_filters.*ShardedCTREngine"):
        ShardedCTREngine(ModelSpec("dnn_pipeline", ccpm_filters=(2,), **KW["dnn_pipeline"]), 64, ex)


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
    """ccpm_filters=C0,C1 is parsed when given, absent from ModelParams.__dict__ (the start-up dump) when
    not, and reaches ModelSpec through _spec_from_args."""
    from deep_learning_amd.local_run import ModelParams
    from deep_learning_amd.models._ctr_model import _spec_from_args
    plain = ModelParams(_argv(tmp_path, "dnn_pipeline"))
    assert "ccpm_filters" not in plain.__dict__
    mp = ModelParams(_argv(tmp_path, "dnn_pipeline", "ccpm_filters=4,4"))
    assert mp.ccpm_filters == [4, 4]
    assert set(mp.__dict__) - set(plain.__dict__) == {"ccpm_filters"}
    assert {k: v for k, v in mp.__dict__.items() if k in plain.__dict__} == plain.__dict__
    assert _spec_from_args("dnn_pipeline", mp).ccpm_filters == (4, 4)
    assert _spec_from_args("dnn_pipeline", plain).ccpm_filters == ()
    assert ModelParams(_argv(tmp_path, "dnn_cate", "ccpm_filters=8")).ccpm_filters == [8]
    assert ModelParams(_argv(tmp_path, "dnn_pipeline", "ccpm_filters=1,2,3", "afm_attention=4")).ccpm_filters == [1, 2, 3]


@pytest.mark.parametrize("alg,v,msg", [("dnn_pipeline", "abc", "not a comma-separated list of integers"),
                                       ("dnn_pipeline", "", "not a comma-separated list of integers"),
                                       ("dnn_pipeline", "2,1.5", "not a comma-separated list of integers"),
                                       ("dnn_pipeline", "0", "must hold 1 to 3 values in \\[1, 8\\]"),
                                       ("dnn_pipeline", "9", "must hold 1 to 3 values in \\[1, 8\\]"),
                                       ("dnn_pipeline", "2,-2", "must hold 1 to 3 values in \\[1, 8\\]"),
                                       ("dnn_pipeline", "2,2,2,2", "must hold 1 to 3 values in \\[1, 8\\]"),
                                       ("deepfm_pipeline", "2", "join the tower")])
def test_local_run_refuses_bad_values(tmp_path, alg, v, msg):
    from deep_learning_amd.local_run import ModelParams
    with pytest.raises(SystemExit, match="ccpm_filters=.*" + msg):
        ModelParams(_argv(tmp_path, alg, "ccpm_filters=" + v))


@pytest.mark.parametrize("E,fields,v", [("12", 26, "2"), ("64", 26, "2"), ("8", 1, "2"), ("8", 65, "2"),
                                        ("8", 3, "2,2"), ("8", 26, "2,2,2,2")])
def test_local_run_refuses_maps_outside_the_limits(tmp_path, E, fields, v):
    from deep_learning_amd.local_run import ModelParams
    with pytest.raises(SystemExit, match="ccpm_filters="):
        ModelParams(_argv(tmp_path, "dnn_pipeline", "ccpm_filters=" + v, E=E, fields=fields))
