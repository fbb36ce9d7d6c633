"""CPU checks of the Bi-Interaction pooling (ModelSpec.bi_interaction): why the kernel
forms q as a prefix chain and not as 1/2 (s^2 - sum e^2), in emulated float32; bi_fwd64 against a literal
transcription of NFM.py:192-197 and the explicit pair loop; bi_bwd64 against autograd and central
differences; the float64 restatement (tests/_bi_ref.py) pinned to the oracle at bi = False; the
all-padding sample; ModelSpec's, the sharded engine's and local_run's refusals; the bi_interaction=
override and the shape of deep_0 that follows from it."""
import types

import numpy as np
import pytest
import torch

from oracle import ctr_ref as R
from tests import _bi_ref as Bi

KW = {"dnn_pipeline": dict(C=5, V=3, S=6, E=8, cate_index_size=300, hidden=[16, 8]),
      "dnn_cate": dict(V=2, S=6, E=8, cate_index_size=300, hidden=[16, 8]),
      "dnn_multi": dict(C=5, V=2, S=4, E=8, cate_index_size=300, hidden=[16, 8],
                        multi_ranges=[[0, 7, "a"], [7, 12, "b"]]),
      "dnn_multi_cate": dict(V=0, S=4, E=8, cate_index_size=300, hidden=[16, 8],
                             multi_ranges=[[0, 5, "a"], [5, 6, "b"]])}
KERNEL_SHAPES = [(2, 4), (3, 8), (26, 16), (33, 8), (64, 32), (5, 64)]


def test_the_prefix_chain_keeps_f32_accuracy_where_the_subtractive_form_cancels():
    """Fields ~ N(0.5, 0.05^2), F = 64, both forms of q in emulated float32: the prefix chain as the kernel
    runs it (its two running sums kept as float pairs, bi_f32(x, "pair")) is within 1e-5 of float64, and
    the subtractive form 1/2 (s^2 - sum e^2) errs at least ten times as much.  Errors are relative to
    max |q|: q ~ 500 there, where one float32 ulp is 3e-5, so no float32 result can be within 1e-5
    absolutely.  Measured (seeds 0 / 1 / 2): chain 5.4e-8 / 5.5e-8 / 5.6e-8, the final rounding of q alone;
    subtractive 7.8e-7 / 7.5e-7 / 7.2e-7; ratio 14.3 / 13.5 / 12.8 (13 to 26 at means 1 to 100).
    The plain one-fma chain, which the kernel does not run, is printed beside them: 4.0e-7, only a factor 2
    below the subtractive form, because with a common mean s^2 ~ F^2 m^2 and sum e^2 ~ F m^2 are a factor F
    apart and cancel little; the subtractive form's worse case is the next test's."""
    rng = np.random.default_rng(0)
    x = (0.5 + 0.05 * rng.standard_normal((256, 64, 16))).astype(np.float32)
    q64 = Bi.bi_fwd64(x)
    chain = np.abs(Bi.bi_f32(x, "pair") - q64).max() / np.abs(q64).max()
    plain = np.abs(Bi.bi_f32(x, True) - q64).max() / np.abs(q64).max()
    sub = np.abs(Bi.bi_f32(x, False) - q64).max() / np.abs(q64).max()
    print("relative f32 error at mean 0.5, F = 64: chain %.3g (plain one-fma chain %.3g), subtractive %.3g"
          % (chain, plain, sub))
    assert chain < 1e-5
    assert sub >= 10 * chain


def test_the_subtractive_form_cancels_where_one_field_dominates():
    """One field of size 100 among 63 fields ~ N(0, 0.05^2) (an outlier embedding): s^2 and sum e^2 are
    both ~ 1e4 and agree to the q ~ 100 sum e_f they differ by, so the subtractive form keeps an ulp of 1e4
    where the chain keeps ulps of q.  Even the plain one-fma chain is within 1e-5 of float64 relative to
    max |q| and the subtractive form at least ten times worse (measured: 2.5e-7 against 4.0e-5); the
    kernel's pair chain is no worse than the plain one."""
    rng = np.random.default_rng(0)
    x = (0.05 * rng.standard_normal((256, 64, 16))).astype(np.float32)
    x[:, 17] = 100.0
    q64 = Bi.bi_fwd64(x)
    chain = np.abs(Bi.bi_f32(x, True) - q64).max() / np.abs(q64).max()
    pair = np.abs(Bi.bi_f32(x, "pair") - q64).max() / np.abs(q64).max()
    sub = np.abs(Bi.bi_f32(x, False) - q64).max() / np.abs(q64).max()
    print("relative f32 error with a dominant field: chain %.3g, pair chain %.3g, subtractive %.3g" % (chain, pair, sub))
    assert chain < 1e-5 and pair <= chain
    assert sub >= 10 * chain


@pytest.mark.parametrize("F,E", KERNEL_SHAPES)
def test_the_f32_chain_stays_inside_the_parity_rule_at_the_kernel_fixture(F, E):
    """At the GPU tests' inputs (fields ~ N(0, 1/2), dq ~ N(0, 1) / B) the float32 evaluation the kernels
    run, q's chain with its sums as float pairs and dx0's addend plainly, is within 1e-5 (absolute) of
    float64: the bound the kernels are held to is reachable.  The plain chain is not at F = 64, E = 32
    (|q| up to ~ 40: 3.2e-5; printed), which is why the kernel carries the pairs."""
    x, dq, _ = Bi.kernel_fixture(300, F, E, seed=1000 * F + E + 300)
    q32 = Bi.bi_f32(x, "pair")
    print("plain f32 chain - fp64 at (F, E) =", (F, E), float(np.abs(Bi.bi_f32(x, True) - Bi.bi_fwd64(x)).max()))
    s = np.zeros((300, E), np.float32)
    for f in range(F):
        s = s + x[:, f]
    de32 = dq[:, None, :] * (s[:, None, :] - x)
    err = dict(q=np.abs(q32 - Bi.bi_fwd64(x)).max(), de=np.abs(de32 - Bi.bi_bwd64(x, dq)).max())
    print("f32 emulation - fp64 at (F, E) =", (F, E), {k: float(v) for k, v in err.items()})
    assert err["q"] < 1e-5 and err["de"] < 1e-5


@pytest.mark.parametrize("F,E", [(2, 4), (3, 8), (7, 4), (26, 16)])
def test_forward_is_the_reference_lines_and_the_pair_sum(F, E):
    x = np.random.default_rng(10 * F + E).standard_normal((5, F, E))
    q = Bi.bi_fwd64(x)
    summed_features_emb = x.sum(1)                              # NFM.py:192 torch.sum(fm_second_order_emb, 1)
    summed_features_emb_square = summed_features_emb * summed_features_emb
    squared_sum_features_emb = (x * x).sum(1)                   # NFM.py:195-196
    fm_second_order = (summed_features_emb_square - squared_sum_features_emb) * 0.5   # NFM.py:197
    np.testing.assert_allclose(q, fm_second_order, rtol=1e-12, atol=1e-13)
    pairs = np.zeros_like(q)
    for f in range(F):
        for g in range(f + 1, F):
            pairs += x[:, f] * x[:, g]
    np.testing.assert_allclose(q, pairs, rtol=1e-12, atol=1e-13)


@pytest.mark.parametrize("F,E", [(2, 4), (3, 8), (7, 4)])
def test_backward_formula_matches_autograd_and_finite_differences(F, E):
    rng = np.random.default_rng(100 * F + E)
    x, r = rng.standard_normal((4, F, E)), rng.standard_normal((4, E))
    de = Bi.bi_bwd64(x, r)
    tx = torch.tensor(x, requires_grad=True)
    s = tx.sum(1)
    ((0.5 * (s * s - (tx * tx).sum(1))) * torch.tensor(r)).sum().backward()
    np.testing.assert_allclose(de, tx.grad.numpy(), rtol=1e-11, atol=1e-13)
    f = lambda xx: float((r * Bi.bi_fwd64(xx)).sum())
    step, want = 1e-6, np.zeros(x.size)
    for i in range(x.size):
        hi, lo = x.copy(), x.copy()
        hi.reshape(-1)[i] += step
        lo.reshape(-1)[i] -= step
        want[i] = (f(hi) - f(lo)) / (2 * step)
    np.testing.assert_allclose(de, want.reshape(x.shape), rtol=1e-6, atol=1e-7 * np.abs(want).max())


@pytest.mark.parametrize("name", list(KW))
def test_restatement_is_the_oracle_without_the_pooling(name):
    """bi = False: logits, loss and every parameter gradient equal ctr_ref.forward / ctr_ref.backward run
    in float64, to float64 rounding."""
    kw = KW[name]
    cfg = R.make_cfg(name, **kw)
    P = Bi.init_params(cfg, np.random.default_rng(3))
    assert set(P) == set(R.init_params(cfg, np.random.default_rng(3)))
    b = Bi.X.make_batch(name, kw, 37, 5)
    got = Bi.forward_backward(cfg, P, b)
    fw = R.forward(cfg, P, b, dtype=np.float64)
    G, _ = R.backward(cfg, P, b, fw, dtype=np.float64)
    np.testing.assert_allclose(got["z"], fw["z"], rtol=1e-12, atol=1e-14)
    assert abs(got["loss"] - fw["loss"]) < 1e-13
    for k in P:
        scale = np.abs(G[k]).max()
        assert scale > 0, k
        np.testing.assert_allclose(got["G"][k], G[k], rtol=0, atol=1e-12 * scale, err_msg=k)


@pytest.mark.parametrize("name", list(KW))
def test_restatement_with_the_pooling(name):
    """bi = True: deep_0 has E more rows, q is bi_fwd64 of the model's own fields and the last E columns
    of x0', the logits move, the regulariser does not, and the table's gradient through q alone is
    bi_bwd64's (the model run with deep_0's other rows zeroed against the formula)."""
    kw = KW[name]
    cfg = R.make_cfg(name, **kw)
    P = Bi.init_params(cfg, np.random.default_rng(3), bi=True)
    E = kw["E"]
    assert P["deep_0"].shape == (Bi.deep_in(cfg, False) + E, kw["hidden"][0])
    b = Bi.X.make_batch(name, kw, 23, 9)
    fw = Bi.forward_backward(cfg, P, b, bi=True)
    assert fw["fields"].shape[1] == Bi.n_fields(cfg)
    np.testing.assert_allclose(fw["q"], Bi.bi_fwd64(fw["fields"]), rtol=1e-12, atol=1e-15)
    np.testing.assert_array_equal(fw["x0"][:, -E:], fw["q"])
    plain = Bi.forward_backward(cfg, dict(P, deep_0=P["deep_0"][:-E]), b)
    np.testing.assert_array_equal(fw["x0"][:, :-E], plain["x0"])
    assert np.abs(plain["z"] - fw["z"]).max() > 1e-6
    assert abs((fw["loss"] - fw["data"]) - (plain["loss"] - plain["data"])) < 1e-15


def test_an_all_padding_sample_has_zero_q_and_zero_gradient():
    x = np.random.default_rng(7).standard_normal((4, 5, 8))
    x[2] = 0.0
    r = np.random.default_rng(8).standard_normal((4, 8))
    assert (Bi.bi_fwd64(x)[2] == 0).all() and (Bi.bi_bwd64(x, r)[2] == 0).all()
    assert (Bi.bi_f32(x, True)[2] == 0).all()
    name, kw = "dnn_cate", KW["dnn_cate"]
    cfg = R.make_cfg(name, **kw)
    P = Bi.init_params(cfg, np.random.default_rng(4), bi=True)
    b = Bi.X.make_batch(name, kw, 9, 2)
    b["cate_feats"] = np.asarray(b["cate_feats"]).copy()
    b["cate_feats"][4] = 0
    fw = Bi.forward_backward(cfg, P, b, bi=True)
    assert (fw["q"][4] == 0).all() and np.abs(fw["q"][[0, 1, 2, 3, 5]]).min() > 0
    assert all(np.isfinite(g).all() for g in fw["G"].values())


# --------------------------------------------------------------------------- the interface
def test_model_spec_accepts_the_dnn_models():
    from deep_learning_amd.engine import ModelSpec
    assert ModelSpec("dnn_pipeline").bi_interaction is False and ModelSpec("deepfm_pipeline").bi_interaction is False
    for name, kw in KW.items():
        off, on = ModelSpec(name, **kw), ModelSpec(name, bi_interaction=True, **kw)
        assert on.bi_interaction is True and on.deep_in == off.deep_in + kw["E"]
        rows = on.x0_ref_rows()
        assert sorted(rows) == list(range(on.deep_in))
        # internally q follows the fields; in the reference order it is last
        FE = on.afm_fields * kw["E"]
        assert list(rows[FE:FE + kw["E"]]) == list(range(off.deep_in, on.deep_in))
        assert list(np.delete(rows, np.arange(FE, FE + kw["E"]))) == list(off.x0_ref_rows())
    sp = ModelSpec("dnn_cate", bi_interaction=True, batch_norm=True, afm_attention=4, cross_layers=2, pos_weight=2.0,
                   **KW["dnn_cate"])
    assert sp.bi_interaction and sp.batch_norm and sp.cross_layers == 2
    assert ModelSpec("dnn_cate", bi_interaction=True, pnn="inner", dropout_keep_deep=[1, 1, 0.7],
                     **KW["dnn_cate"]).dropout == [1.0, 1.0, 0.7]
    for over in (dict(S=64, E=64), dict(S=2, E=4), dict(E=12)):
        assert ModelSpec("dnn_pipeline", **dict(KW["dnn_pipeline"], bi_interaction=True, **over)).bi_interaction


@pytest.mark.parametrize("model", ["deepfm_pipeline", "deepfm_cate", "deepfm_multi_cate", "deepfm_multi", "wdl",
                                   "dnn", "deepfm"])
def test_model_spec_refuses_other_models(model):
    from deep_learning_amd.engine import ModelSpec
    with pytest.raises(ValueError, match="bi_interaction: the Bi-Interaction pooling feeds the tower of"):
        ModelSpec(model, bi_interaction=True)
    assert ModelSpec(model, bi_interaction=False).bi_interaction is False


def test_model_spec_refuses_what_the_pooling_cannot_take():
    from deep_learning_amd.engine import ModelSpec
    kw = KW["dnn_pipeline"]
    with pytest.raises(ValueError, match="bi_interaction: not supported with tower='bf16'"):
        ModelSpec("dnn_pipeline", bi_interaction=True, tower="bf16", **kw)
    with pytest.raises(ValueError, match="bi_interaction: not supported with tower-input dropout"):
        ModelSpec("dnn_pipeline", bi_interaction=True, dropout_keep_deep=[0.9, 1, 1], **kw)
    for over in (dict(S=1), dict(S=65), dict(E=6), dict(E=68), dict(E=2)):
        with pytest.raises(ValueError, match=r"bi_interaction: 2 to 64 embedded fields of a size that is a multiple "
                                             r"of 4 in \[4, 64\]"):
            ModelSpec("dnn_pipeline", **dict(kw, bi_interaction=True, **over))
    with pytest.raises(ValueError, match="bi_interaction"):       # 63 singles + 2 pooled = 65 fields
        ModelSpec("dnn_multi", **dict(KW["dnn_multi"], bi_interaction=True, S=63))


def test_sharded_engine_refuses():
    """Before anything touches a device or the exchange."""
    from deep_learning_amd.engine import ModelSpec
    from deep_learning_amd.shard import ShardedCTREngine
    ex = types.SimpleNamespace(world=1, rank=0)
    with pytest.raises(ValueError, match="bi_interaction: not supported by ShardedCTREngine"):
        ShardedCTREngine(ModelSpec("dnn_pipeline", bi_interaction=True, **KW["dnn_pipeline"]), 64, ex)


@pytest.mark.parametrize("name", list(KW))
def test_parameters_of_the_other_width_are_refused(name):
    """What CTREngine.load_params (and so load_model and a checkpoint's restore) asks first."""
    from deep_learning_amd.engine import ModelSpec
    kw = KW[name]
    cfg = R.make_cfg(name, **kw)
    P_off = Bi.init_params(cfg, np.random.default_rng(1))
    P_on = Bi.init_params(cfg, np.random.default_rng(1), bi=True)
    off, on = ModelSpec(name, **kw), ModelSpec(name, bi_interaction=True, **kw)
    off.check_deep0(P_off)
    on.check_deep0(P_on)
    with pytest.raises(ValueError, match="deep_0 has %d rows for %d .*bi_interaction=True" % (off.deep_in, on.deep_in)):
        on.check_deep0(P_off)
    with pytest.raises(ValueError, match="deep_0 has %d rows for %d .*bi_interaction=False" % (on.deep_in, off.deep_in)):
        off.check_deep0(P_on)


def _argv(tmp_path, alg, *over):
    conf = tmp_path / "conf"
    if not conf.exists():
        conf.mkdir()
        lines = ["f%d\tx\tfloat" % i for i in range(13)] + ["c%d\tx\tstring" % i for i in range(26)]
        (conf / "dnn.conf").write_text("\n".join(lines) + "\n")
    return ["local_run.py", alg, "train", "1", "8", "3000", "3", str(conf), "tr/", "pr/", "pb", "ck", "0", "ck",
            "batch_size=64"] + list(over)


def test_local_run_override(tmp_path):
    """bi_interaction=1 is parsed when given, absent from ModelParams.__dict__ (the start-up dump) when
    not, and reaches ModelSpec through _spec_from_args, where deep_in grows by E."""
    from deep_learning_amd.local_run import ModelParams
    from deep_learning_amd.models._ctr_model import _spec_from_args
    plain = ModelParams(_argv(tmp_path, "dnn_pipeline"))
    assert "bi_interaction" not in plain.__dict__
    mp = ModelParams(_argv(tmp_path, "dnn_pipeline", "bi_interaction=1", "batch_norm=1"))
    assert mp.bi_interaction is True
    assert set(mp.__dict__) - set(plain.__dict__) == {"bi_interaction", "batch_norm"}
    on, off = _spec_from_args("dnn_pipeline", mp), _spec_from_args("dnn_pipeline", plain)
    assert on.bi_interaction is True and on.batch_norm is True and off.bi_interaction is False
    assert on.deep_in == off.deep_in + 8 == 13 + 26 * 8 + 8
    assert _spec_from_args("dnn_pipeline", ModelParams(_argv(tmp_path, "dnn_pipeline", "bi_interaction=0"))
                           ).bi_interaction is False


@pytest.mark.parametrize("alg,v,msg", [("dnn_pipeline", "2", "must be 0 or 1"), ("dnn_pipeline", "", "must be 0 or 1"),
                                       ("dnn_pipeline", "true", "must be 0 or 1"),
                                       ("deepfm_pipeline", "1", "feeds the tower"), ("wdl", "1", "feeds the tower")])
def test_local_run_refuses_bad_values(tmp_path, alg, v, msg):
    from deep_learning_amd.local_run import ModelParams
    with pytest.raises(SystemExit, match="bi_interaction=.*" + msg):
        ModelParams(_argv(tmp_path, alg, "bi_interaction=" + v))
