"""CPU checks of batch normalisation in the deep tower (ModelSpec.batch_norm): the float64
restatement (tests/_bn_ref.py) pinned to the oracle at batch_norm = False for one model of each
family, bn_fwd64 and the running recurrence against torch.nn.functional.batch_norm, bn_bwd64 against
autograd and central differences, the float32 emulation that shows the cancellation case separates a
raw-moment variance from a centred one, every refusal by message and local_run's overrides."""
import types

import numpy as np
import pytest
import torch

from oracle import ctr_ref as R
from tests import _bn_ref as Bn

KW = {"deepfm_pipeline": dict(C=5, V=3, S=6, E=8, cate_index_size=300, hidden=[16, 8]),
      "dnn_pipeline": dict(C=5, V=3, S=6, E=8, cate_index_size=300, hidden=[16, 8]),
      "dnn_multi_cate": dict(V=0, S=4, E=8, cate_index_size=300, hidden=[16, 8],
                             multi_ranges=[[0, 5, "a"], [5, 6, "b"]]),
      "deepfm_multi": dict(C=4, V=2, S=4, E=8, cate_index_size=300, hidden=[16, 8],
                           multi_ranges=[[0, 7, "a"], [7, 12, "b"]]),
      "wdl": dict(C=5, S=6, E=8, cate_index_size=300, hidden=[16, 8], Fw=4)}


@pytest.mark.parametrize("name", list(KW))
def test_restatement_is_the_oracle_without_batch_norm(name):
    """batch_norm = False: logits, loss and every parameter gradient equal ctr_ref.forward /
    ctr_ref.backward run in float64, to float64 rounding."""
    kw = KW[name]
    cfg = R.make_cfg(name, **kw)
    P = Bn.init_params(cfg, 0, 0, False, np.random.default_rng(3))
    assert set(P) == set(R.init_params(cfg, np.random.default_rng(3)))
    b = Bn.make_batch(name, kw, 37, 5)
    got = Bn.forward_backward(cfg, P, b)
    fw = R.forward(cfg, P, b, dtype=np.float64)
    G, _ = R.backward(cfg, P, b, fw, dtype=np.float64)
    np.testing.assert_allclose(got["z"], fw["z"], rtol=1e-12, atol=1e-14)
    assert abs(got["loss"] - fw["loss"]) < 1e-13
    for k in P:
        scale = np.abs(G[k]).max()
        assert scale > 0, k
        np.testing.assert_allclose(got["G"][k], G[k], rtol=0, atol=1e-12 * scale, err_msg=k)


def test_restatement_with_the_branches_is_the_afm_restatement_without_batch_norm():
    name, kw = "dnn_pipeline", KW["dnn_pipeline"]
    cfg = R.make_cfg(name, **kw)
    P = Bn.init_params(cfg, 2, 3, False, np.random.default_rng(4))
    b = Bn.make_batch(name, kw, 23, 6)
    got, want = Bn.forward_backward(cfg, P, b, 2, 3), Bn.Af.forward_backward(cfg, P, b, 2, 3)
    np.testing.assert_allclose(got["z"], want["z"], rtol=1e-13, atol=1e-15)
    for k in P:
        np.testing.assert_allclose(got["G"][k], want["G"][k], rtol=1e-10, atol=1e-16, err_msg=k)


@pytest.mark.parametrize("m", [0.1, 1.0])
def test_forward_and_running_update_are_torchs(m):
    """bn_fwd64 and running_update equal torch.nn.functional.batch_norm in float64: training mode
    (batch statistics, the running ones updated with the unbiased variance) and eval mode."""
    c, gamma, beta, _, rm, rv = (np.asarray(a, np.float64) for a in Bn.kernel_fixture(37, 11, 5))
    t = torch.tensor
    trm, trv = t(rm.copy()), t(rv.copy())
    y = torch.nn.functional.batch_norm(t(c), trm, trv, t(gamma), t(beta), True, m, Bn.EPS).numpy()
    fw = Bn.bn_fwd64(c, gamma, beta)
    np.testing.assert_allclose(fw["y"], y, rtol=1e-12, atol=1e-13)
    nrm, nrv = Bn.running_update(rm, rv, fw["mu"], fw["var"], 37, m)
    np.testing.assert_allclose(nrm, trm.numpy(), rtol=1e-13, atol=1e-15)
    np.testing.assert_allclose(nrv, trv.numpy(), rtol=1e-13, atol=1e-15)
    assert np.abs(nrm - rm).max() > 1e-3
    ye = torch.nn.functional.batch_norm(t(c), t(rm), t(rv), t(gamma), t(beta), False, m, Bn.EPS).numpy()
    fe = Bn.bn_fwd64(c, gamma, beta, running=(rm, rv))
    np.testing.assert_allclose(fe["y"], ye, rtol=1e-12, atol=1e-13)
    assert np.abs(ye - y).max() > 1e-2
    np.testing.assert_array_equal(fe["h"], np.maximum(fe["y"], 0))


def test_backward_formulas_match_autograd_and_finite_differences():
    c, gamma, beta, r, _, _ = (np.asarray(a, np.float64) for a in Bn.kernel_fixture(9, 5, 8))
    fw = Bn.bn_fwd64(c, gamma, beta)
    dc, dg, db = Bn.bn_bwd64(r, fw["xhat"], gamma, fw["invstd"])
    tc, tg, tb = (torch.tensor(a, requires_grad=True) for a in (c, gamma, beta))
    y = torch.nn.functional.batch_norm(tc, None, None, tg, tb, True, 0.1, Bn.EPS)
    (y * torch.tensor(r)).sum().backward()
    for got, want in ((dc, tc.grad), (dg, tg.grad), (db, tb.grad)):
        np.testing.assert_allclose(got, want.numpy(), rtol=1e-10, atol=1e-14)
    f = lambda cc: float((r * Bn.bn_fwd64(cc, gamma, beta)["y"]).sum())
    step, want = 1e-6, np.zeros(c.size)
    for i in range(c.size):
        hi, lo = c.copy(), c.copy()
        hi.reshape(-1)[i] += step
        lo.reshape(-1)[i] -= step
        want[i] = (f(hi) - f(lo)) / (2 * step)
    np.testing.assert_allclose(dc, want.reshape(c.shape), rtol=1e-5, atol=1e-8 * np.abs(want).max())


def test_restatement_gradients_and_running_statistics():
    """With batch_norm the autograd model's gamma / beta gradients are nonzero, the running ones get
    none, a training step moves the running statistics by the recurrence and eval mode reads them."""
    name, kw = "deepfm_pipeline", KW["deepfm_pipeline"]
    cfg = R.make_cfg(name, **kw)
    P = Bn.init_params(cfg, 0, 0, True, np.random.default_rng(8), jitter=0.2)
    assert set(Bn.bn_keys(cfg)) <= set(P) and len(Bn.bn_keys(cfg)) == 8
    b = Bn.make_batch(name, kw, 23, 9)
    opt = R.AdamTF1(cfg, P)
    P0 = {k: v.copy() for k, v in P.items()}
    fw = Bn.train_step(cfg, P, opt, b)
    for k in Bn.bn_keys(cfg, running=False):
        assert np.abs(fw["G"][k]).max() > 0 and np.abs(P[k] - P0[k]).max() > 0, k
    for l in range(2):
        mu, var = fw["stats"][l]
        np.testing.assert_allclose(P[Bn.KEY % (l + 1, "running_mean")], 0.1 * mu, rtol=1e-6, atol=1e-8)
        np.testing.assert_allclose(P[Bn.KEY % (l + 1, "running_var")], 0.9 + 0.1 * var * 23 / 22, rtol=1e-6)
        assert (fw["G"][Bn.KEY % (l + 1, "running_mean")] == 0).all()
    ev = Bn.forward_backward(cfg, P, b, bn=True, train=False)
    tr = Bn.forward_backward(cfg, P, b, bn=True, train=True)
    assert np.abs(ev["z"] - tr["z"]).max() > 1e-3
    plain = Bn.forward_backward(cfg, {k: v for k, v in P.items() if not k.startswith("batch_norm")}, b)
    assert abs((tr["loss"] - tr["data"]) - (plain["loss"] - plain["data"])) < 1e-15


def test_cancellation_case_separates_raw_from_centred_variance():
    """The GPU test's cancellation case (B = 300, D = 400, every column offset by 1,000, std in
    [0.25, 4]) in a float32 numpy emulation: xhat from a centred variance stays within the test's bound
    (1e-5 absolute against float64 on the f32-rounded c, the mean taken exactly), from E[c^2] - mu^2 it
    misses it by orders of magnitude — so the test does tell the two forms apart."""
    c = Bn.kernel_fixture(300, 400, 77, offset=1000.0)[0]
    ref = Bn.bn_fwd64(c, np.ones(400), np.zeros(400))
    assert 0.2 < np.sqrt(ref["var"]).min() and np.sqrt(ref["var"]).max() < 4.5
    err = {}
    for centred in (True, False):
        _, var = Bn.var_f32(c, centred)
        inv = 1.0 / np.sqrt(np.maximum(var.astype(np.float64), 0) + Bn.EPS)
        err[centred] = np.abs((c.astype(np.float64) - ref["mu"]) * inv - ref["xhat"]).max()
    assert err[True] < 1e-5 < 1e-2 < err[False], err


def test_model_spec_defaults_and_acceptance():
    from deep_learning_amd.engine import ModelSpec
    for name, kw in KW.items():
        sp = ModelSpec(name, **kw)
        assert sp.batch_norm is False and sp.bn_eps == 1e-5 and sp.bn_momentum == 0.1
        sp = ModelSpec(name, batch_norm=True, bn_eps=1e-3, bn_momentum=1.0, **kw)
        assert sp.batch_norm is True and sp.bn_eps == 1e-3 and sp.bn_momentum == 1.0
    sp = ModelSpec("dnn_pipeline", batch_norm=True, cross_layers=2, afm_attention=4, pos_weight=2.0,
                   **KW["dnn_pipeline"])
    assert sp.batch_norm and sp.cross_layers == 2 and sp.afm_attention == 4
    sp = ModelSpec("dnn_pipeline", batch_norm=True, dropout_keep_deep=[0.8, 1, 1], **KW["dnn_pipeline"])
    assert sp.batch_norm and sp.dropout == [0.8, 1.0, 1.0]                    # tower-input dropout stays allowed
    assert ModelSpec("deepfm_pipeline", batch_norm=True, dropout_keep_fm=[0.9, 0.9], **KW["deepfm_pipeline"]).batch_norm


def test_model_spec_refusals():
    from deep_learning_amd.engine import ModelSpec
    kw = KW["dnn_pipeline"]
    with pytest.raises(ValueError, match="batch_norm: not supported with tower='bf16'"):
        ModelSpec("dnn_pipeline", batch_norm=True, tower="bf16", **kw)
    for keep in ([1, 0.9, 1], [1, 1, 0.9]):
        with pytest.raises(ValueError, match="batch_norm: not supported with dropout on a hidden layer's output"):
            ModelSpec("dnn_pipeline", batch_norm=True, dropout_keep_deep=keep, **kw)
    with pytest.raises(ValueError, match="batch_norm: not supported together with pnn"):
        ModelSpec("dnn_pipeline", batch_norm=True, pnn="inner", **kw)
    for bad in (0.0, -1e-5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="batch_norm: bn_eps must be finite and > 0"):
            ModelSpec("dnn_pipeline", batch_norm=True, bn_eps=bad, **kw)
    for bad in (0.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match=r"batch_norm: bn_momentum must lie in \(0, 1\]"):
            ModelSpec("dnn_pipeline", batch_norm=True, bn_momentum=bad, **kw)


def test_sharded_engine_refuses():
    """Before anything touches a device or the exchange."""
    from deep_learning_amd.engine import ModelSpec
    from deep_learning_amd.shard import ShardedCTREngine
    ex = types.SimpleNamespace(world=1, rank=0)
    with pytest.raises(ValueError, match="batch_norm: not supported by ShardedCTREngine"):
        ShardedCTREngine(ModelSpec("dnn_pipeline", batch_norm=True, **KW["dnn_pipeline"]), 64, ex)


def _argv(tmp_path, alg, *over):
    conf = tmp_path / "conf"
    if not conf.exists():
        conf.mkdir()
        lines = ["f%d\tx\tfloat" % i for i in range(13)] + ["c%d\tx\tstring" % i for i in range(26)]
        (conf / "dnn.conf").write_text("\n".join(lines) + "\n")
    return ["local_run.py", alg, "train", "1", "8", "3000", "3", str(conf), "tr/", "pr/", "pb", "ck", "0", "ck",
            "batch_size=64"] + list(over)


def test_local_run_overrides(tmp_path):
    """batch_norm=1 bn_eps= bn_momentum= are parsed when given, absent from ModelParams.__dict__ (the
    start-up dump) when not, and reach ModelSpec through _spec_from_args."""
    from deep_learning_amd.local_run import ModelParams
    from deep_learning_amd.models._ctr_model import _spec_from_args
    plain = ModelParams(_argv(tmp_path, "deepfm_pipeline"))
    assert not {"batch_norm", "bn_eps", "bn_momentum"} & set(plain.__dict__)
    mp = ModelParams(_argv(tmp_path, "deepfm_pipeline", "batch_norm=1", "bn_eps=1e-3", "bn_momentum=0.2"))
    assert mp.batch_norm is True and mp.bn_eps == 1e-3 and mp.bn_momentum == 0.2
    assert set(mp.__dict__) - set(plain.__dict__) == {"batch_norm", "bn_eps", "bn_momentum"}
    assert {k: v for k, v in mp.__dict__.items() if k in plain.__dict__} == plain.__dict__
    sp = _spec_from_args("deepfm_pipeline", mp)
    assert sp.batch_norm is True and sp.bn_eps == 1e-3 and sp.bn_momentum == 0.2
    assert _spec_from_args("deepfm_pipeline", plain).batch_norm is False
    off = ModelParams(_argv(tmp_path, "dnn_pipeline", "batch_norm=0"))
    assert off.batch_norm is False and _spec_from_args("dnn_pipeline", off).batch_norm is False


@pytest.mark.parametrize("kv,msg", [("batch_norm=yes", "must be 0 or 1"), ("bn_eps=0", "finite and > 0"),
                                    ("bn_eps=x", "not a number"), ("bn_momentum=0", r"lie in \(0, 1\]"),
                                    ("bn_momentum=1.5", r"lie in \(0, 1\]")])
def test_local_run_refuses_bad_values(tmp_path, kv, msg):
    from deep_learning_amd.local_run import ModelParams
    with pytest.raises(SystemExit, match=msg):
        ModelParams(_argv(tmp_path, "dnn_pipeline", kv))
