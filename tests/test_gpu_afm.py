"""GPU checks of the attentional pairwise interactions (ModelSpec.afm_attention, csrc/afm.hip,
DESIGN 4l): dl_afm_fwd / dl_afm_bwd against the float64 formulas (tests/_afm_ref.py) on the dyadic
fixture; five-step trajectories of the four dnn_* models against the float64 restatement in every
table mode, with the cross network, with hidden-layer dropout and with sample weights; predict,
checkpoint, export and local_run; and the unchanged kernel sequence at afm_attention = 0.

Kernel shapes (F, E, A): (2, 8, 1) the smallest; (3, 16, 5) odd F, unaligned A; (26, 16, 16) and
(32, 16, 16) two samples a wave, odd and even round counts; (33, 8, 32) one sample a wave, the
largest A; (64, 32, 7) the largest F and E, 2,016 pairs; B = 1, 63, 300 (a partial last group, more
than one pass of the backward's capped grid)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from deep_learning_amd import _lib
from deep_learning_amd._lib import call, ptr
from deep_learning_amd.engine import CTREngine, ModelSpec
from oracle import ctr_ref as R
from tests import _afm_ref as Af
from tests import _dropout_ref as D
from tests import _sample_weight_ref as W

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-5          # tests/test_gpu_parity.py: absolute, on logits and dense gradients / parameters
AT = 4
KW = {"dnn_pipeline": dict(C=13, V=3, S=8, E=8, cate_index_size=1000, hidden=[32, 16]),
      "dnn_cate": dict(V=2, S=8, E=8, cate_index_size=1000, hidden=[32, 16]),
      "dnn_multi": dict(C=5, V=2, S=4, E=8, cate_index_size=1000, hidden=[32, 16],
                        multi_ranges=[[0, 7, "a"], [7, 12, "b"]]),
      "dnn_multi_cate": dict(V=0, S=4, E=8, cate_index_size=1000, hidden=[32, 16],
                             multi_ranges=[[0, 5, "a"], [5, 6, "b"]])}
MODES = {"atomic": dict(bwd="atomic"), "sorted": dict(bwd="sorted"), "lazy": dict(adam="lazy")}
B_ = 64
SHAPES = [(2, 8, 1), (3, 16, 5), (26, 16, 16), (32, 16, 16), (33, 8, 32), (64, 32, 7)]


def _s():
    return _lib.stream_handle()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


# --------------------------------------------------------------------------- 1. the kernels
def _run_kernels(fx, ld_extra=5, dx_col0=0, z_add=None, runs=1):
    """dl_afm_fwd then dl_afm_bwd on a fixture; x0 [B, F E + ld_extra] (pad 7.0, never read), dx0
    pre-filled and wider than the field range.  Returns per run (z, stats, dx, slab) and the pre-fill."""
    x, p, h, b, Wm, dz = fx
    B, F, E = x.shape
    A = len(h)
    ld = F * E + ld_extra
    x0 = np.full((B, ld), 7.0, np.float32)
    x0[:, :F * E] = x.reshape(B, F * E)
    dx_ld = dx_col0 + F * E + 3
    pre = (np.random.default_rng(5).standard_normal((B, dx_ld)) * 0.1).astype(np.float32)
    dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in
           dict(x0=x0, prm=Af.pack(p, h, b, Wm), dz=dz).items()}
    za = torch.from_numpy(z_add).cuda() if z_add is not None else None
    grid = _lib.lib().dl_afm_grid(B)
    n = E + 2 * A + E * A
    outs = []
    for _ in range(runs):
        z = torch.full((B + 1,), -7.0, device="cuda")
        st = torch.full((B + 1, 2), -7.0, device="cuda")
        dx = torch.from_numpy(pre).cuda()
        slab = torch.full((grid + 1, n), -7.0, device="cuda")
        call("dl_afm_fwd", B, F, E, A, ptr(dev["x0"]), ld, 0, ptr(dev["prm"]), ptr(za), ptr(st), ptr(z), _s())
        call("dl_afm_bwd", B, F, E, A, ptr(dev["x0"]), ld, 0, ptr(dev["prm"]), ptr(st), ptr(dev["dz"]), ptr(dx), dx_ld,
             dx_col0, ptr(slab), grid, _s())
        torch.cuda.synchronize()
        outs.append(tuple(t.cpu().numpy() for t in (z, st, dx, slab)))
    return outs, pre, grid


def _errors(fx, out, pre, grid, dx_col0, z_add=None):
    x, p, h, b, Wm, dz = fx
    B, F, E = x.shape
    z64, st64, _, _, _ = Af.afm_fwd64(x, p, h, b, Wm)
    ddx, dp, dh, db, dW = Af.afm_bwd64(x, p, h, b, Wm, dz)
    zg, sg, dxg, slg = out
    assert zg[B] == -7 and (sg[B] == -7).all() and (slg[grid] == -7).all()
    lo, hi = dx_col0, dx_col0 + F * E
    assert np.array_equal(_bits(dxg[:, :lo]), _bits(pre[:, :lo])) and np.array_equal(_bits(dxg[:, hi:]), _bits(pre[:, hi:]))
    assert np.abs(ddx).max() > 0
    want = np.concatenate([dp, dh, db, dW.reshape(-1)])
    zref = z64 + (0 if z_add is None else z_add.astype(np.float64))
    ref_max = max(np.abs(zref).max(), np.abs(ddx).max(), np.abs(want).max())
    return dict(z=np.abs(zg[:B] - zref).max(), smax=np.abs(sg[:B, 0] - st64[:, 0]).max(),
                dx0=np.abs(dxg[:, lo:hi] - (pre[:, lo:hi].astype(np.float64) + ddx.reshape(B, F * E))).max(),
                slab=np.abs(slg[:grid].astype(np.float64).sum(0) - want).max()), ref_max


@pytest.mark.parametrize("B", [1, 63, 300])
@pytest.mark.parametrize("F,E,A", SHAPES)
def test_afm_kernels_match_fp64(hip_lib, F, E, A, B):
    """z, dx0's addend and the slab's column sums (dp, dh, db, dW) within 1e-5 (absolute) of the
    float64 formulas on the dyadic fixture (every u exact: no ReluGrad decision can differ); dx0 is
    pre-filled, added into, and its columns outside the fields keep their bits (the fields start at
    column 3 of dx0 in the (3, 16, 5) case); two runs give the same bits; z_add given equals z_add
    NULL plus the addend, bit for bit.  Measured worst errors: DESIGN 4l."""
    fx = Af.dyadic_fixture(B, F, E, A, seed=1000 * F + 10 * A + B)
    col0 = 3 if F == 3 else 0
    outs, pre, grid = _run_kernels(fx, dx_col0=col0, runs=2)
    assert 1 <= grid <= 512 and _lib.lib().dl_afm_grid(1 << 20) == 512
    for a, b in zip(outs[0], outs[1]):
        assert np.array_equal(_bits(a), _bits(b))
    err, _ = _errors(fx, outs[0], pre, grid, col0)
    print("max |kernel - fp64|:", {k: float(v) for k, v in err.items()})
    for k in ("z", "dx0", "slab"):
        assert err[k] < TOL, (k, err[k])
    za = np.random.default_rng(B).standard_normal(B).astype(np.float32)
    (with_add,), _, _ = _run_kernels(fx, dx_col0=col0, z_add=za)
    assert np.array_equal(_bits(with_add[0][:B]), _bits(outs[0][0][:B] + za))
    for a, b in zip(with_add[1:], outs[0][1:]):
        assert np.array_equal(_bits(a), _bits(b))


def test_afm_kernels_survive_scores_beyond_the_f32_exp_range(hip_lib):
    """h scaled by 50: scores reach far beyond 88, where a bare f32 exp overflows; the outputs are
    finite and within 1e-5 of the float64 formulas relative to max(1, max |ref|)."""
    fx = Af.dyadic_fixture(63, 26, 16, 16, seed=77, h_scale=50.0)
    _, st64, _, _, _ = Af.afm_fwd64(*fx[:5])
    assert st64[:, 0].max() > 200
    outs, pre, grid = _run_kernels(fx)
    assert all(np.isfinite(a[:-1]).all() for a in outs[0])
    err, ref_max = _errors(fx, outs[0], pre, grid, 0)
    print("max |kernel - fp64|:", {k: float(v) for k, v in err.items()}, "max |ref|", float(ref_max))
    for k in ("z", "dx0", "slab"):
        assert err[k] < TOL * max(1.0, ref_max), (k, err[k])


def test_afm_kernels_refuse_what_they_cannot_take(hip_lib):
    t = torch.full((8, 2200), 3.0, device="cuda")
    prm = torch.zeros(2048, device="cuda")
    out = torch.full((64,), 3.0, device="cuda")
    slab = torch.full((2048,), 3.0, device="cuda")
    for F, E, A in ((1, 8, 4), (65, 8, 4), (4, 12, 4), (4, 8, 0), (4, 8, 33)):
        with pytest.raises(_lib.DLError, match="F %d fields|E %d not|A %d attention" % (F, E, A)):
            call("dl_afm_fwd", 8, F, E, A, ptr(t), 2200, 0, ptr(prm), None, ptr(out), ptr(out), _s())
        with pytest.raises(_lib.DLError, match="F %d fields|E %d not|A %d attention" % (F, E, A)):
            call("dl_afm_bwd", 8, F, E, A, ptr(t), 2200, 0, ptr(prm), ptr(out), ptr(out), ptr(t), 2200, 0, ptr(slab), 1,
                 _s())
    with pytest.raises(_lib.DLError, match="field columns"):     # fields past x0's row
        call("dl_afm_fwd", 8, 4, 8, 4, ptr(t), 2200, 2190, ptr(prm), None, ptr(out), ptr(out), _s())
    with pytest.raises(_lib.DLError, match="dx0 columns"):
        call("dl_afm_bwd", 8, 4, 8, 4, ptr(t), 2200, 0, ptr(prm), ptr(out), ptr(out), ptr(t), 2200, 2190, ptr(slab), 1, _s())
    with pytest.raises(_lib.DLError, match="slab needs"):
        call("dl_afm_bwd", 64, 4, 8, 4, ptr(t), 2200, 0, ptr(prm), ptr(out), ptr(out), ptr(t), 2200, 0, ptr(slab), 1, _s())
    torch.cuda.synchronize()
    assert (t == 3).all() and (out == 3).all() and (slab == 3).all()


# --------------------------------------------------------------------------- 2. the engine
def _batches(name, n, seed=11, B=B_):
    return [Af.X.make_batch(name, KW[name], B, seed + i) for i in range(n)]


def _init(name, L, seed):
    """Injected parameters at the models' init scales."""
    cfg = R.make_cfg(name, **KW[name])
    P = Af.init_params(cfg, L, AT, np.random.default_rng(seed))
    assert np.abs(P["attention_b"]).min() > 1e-3          # u ~ b at this scale: no kink within rounding
    return cfg, P


def _ref_run(name, P0, bs, L=0, **kw):
    cfg = R.make_cfg(name, **KW[name])
    P = {k: v.copy() for k, v in P0.items()}
    opt = R.AdamTF1(cfg, P)
    zs, losses = [], []
    for i, b in enumerate(bs):
        fw = Af.train_step(cfg, P, opt, b, L, AT, **(kw["per_step"](i, b) if "per_step" in kw else {}))
        zs.append(fw["z"])
        losses.append(fw["loss"])
    return zs, losses, P


@pytest.fixture(scope="module")
def trajectories():
    """The restatement's five steps from injected parameters, once per model."""
    out = {}
    for name in KW:
        _, P0 = _init(name, 0, 42)
        bs = _batches(name, 5)
        out[name] = (P0, bs) + _ref_run(name, P0, bs)
    return out


def _run(eng, bs, graph_from=2):
    zs, losses = [], []
    for i, b in enumerate(bs):
        eng.train_step(b, graph=i >= graph_from)
        torch.cuda.synchronize()
        zs.append(eng.z[: eng.last_batch].cpu().numpy().copy())
        losses.append(eng.loss())
    eng.check_error()
    return zs, losses


def _check(eng, got_z, got_l, zs, losses, P, tag):
    err = dict(z=max(np.abs(a - b).max() for a, b in zip(got_z, zs)),
               loss=max(abs(a - b) for a, b in zip(got_l, losses)))
    got = eng.params()
    assert set(got) == set(P)
    for k in Af.AFM_KEYS:
        assert got[k].shape == P[k].shape, k
    err["params"] = max(np.abs(got[k] - P[k]).max() for k in P)
    err["attention"] = max(np.abs(got[k] - P[k]).max() for k in Af.AFM_KEYS)
    print(tag, "max |engine - restatement|:", {k: float(v) for k, v in err.items()})
    for k, v in err.items():
        assert v < TOL, (k, v)
    return got


@pytest.mark.parametrize("name", list(KW))
def test_trajectory_matches_restatement(hip_lib, trajectories, name):
    """Five steps (two eager, three replayed as a hipGraph) in every table mode: each step's
    logits and loss and the final parameters (the four attention variables among them) within 1e-5
    of the restatement; lazy and sorted + dense bit for bit (dnn_pipeline, dnn_cate: the multi-hot
    models' dense pooled scatter is atomic)."""
    P0, bs, zs, losses, P = trajectories[name]
    res = {}
    for mode, ekw in MODES.items():
        eng = CTREngine(ModelSpec(name, afm_attention=AT, **KW[name]), max_batch=B_, init="none", **ekw)
        eng.load_params({k: v.copy() for k, v in P0.items()})
        gz, gl = _run(eng, bs)
        res[mode] = (gz, _check(eng, gz, gl, zs, losses, P, "%s %s" % (name, mode)), eng.dense_state())
    for mv in ("m", "v"):
        for k in Af.AFM_KEYS:
            assert np.abs(res["lazy"][2][mv][k]).max() > 0
    if "multi_ranges" not in KW[name]:
        for a, b in zip(res["lazy"][0], res["sorted"][0]):
            np.testing.assert_array_equal(a, b)
        for k in res["lazy"][1]:
            np.testing.assert_array_equal(res["lazy"][1][k], res["sorted"][1][k], err_msg=k)
        for mv in ("m", "v"):
            for k in Af.AFM_KEYS:
                np.testing.assert_array_equal(res["lazy"][2][mv][k], res["sorted"][2][mv][k], err_msg=k)
    # the branch does matter: the same steps without it end elsewhere
    plain = CTREngine(ModelSpec(name, **KW[name]), max_batch=B_, init="none", adam="lazy")
    plain.load_params({k: v.copy() for k, v in P0.items() if k not in Af.AFM_KEYS})
    plain.train_step(bs[0])
    torch.cuda.synchronize()
    assert np.abs(plain.z[:B_].cpu().numpy() - zs[0]).max() > 5 * TOL      # (z_afm ~ 1e-4 at the init scale)
    assert max(np.abs(P[k] - P0[k]).max() for k in Af.AFM_KEYS) > 100 * TOL


def test_with_the_cross_network(hip_lib):
    """dnn_multi with cross_layers = 2 as well: z_cross rides in through z_add."""
    name = "dnn_multi"
    _, P0 = _init(name, 2, 43)
    bs = _batches(name, 5, seed=15)
    zs, losses, P = _ref_run(name, P0, bs, L=2)
    eng = CTREngine(ModelSpec(name, afm_attention=AT, cross_layers=2, **KW[name]), max_batch=B_, init="none", adam="lazy")
    eng.load_params({k: v.copy() for k, v in P0.items()})
    gz, gl = _run(eng, bs)
    _check(eng, gz, gl, zs, losses, P, "cross + afm")


def test_same_seed_runs_agree_bit_for_bit(hip_lib):
    """Device-initialised engines of one seed, five graph steps each: logits, every parameter and
    the attention moments equal bit for bit; the attention variables are drawn at their reference
    scales and shapes."""
    name = "dnn_multi"
    bs = _batches(name, 5, seed=3)
    out = []
    for _ in range(2):
        eng = CTREngine(ModelSpec(name, afm_attention=16, **KW[name]), max_batch=B_, seed=7, adam="lazy")
        p0 = eng.params()
        zs, _ = _run(eng, bs, graph_from=0)
        out.append((zs, eng.params(), eng.dense_state(), p0))
    for a, b in zip(out[0][0], out[1][0]):
        np.testing.assert_array_equal(a, b)
    for k in out[0][1]:
        np.testing.assert_array_equal(out[0][1][k], out[1][1][k], err_msg=k)
    for k in Af.AFM_KEYS:
        np.testing.assert_array_equal(out[0][2]["v"][k], out[1][2]["v"][k], err_msg=k)
    p0, E = out[0][3], KW[name]["E"]
    shapes = dict(attention_w=(E, 16), attention_b=(1, 16), attention_h=(1, 16), attention_p=(E, 1))
    for k, shp in shapes.items():
        want = np.sqrt(2.0 / (16 + E)) if k in ("attention_w", "attention_b") else 1.0
        assert p0[k].shape == shp and 0.5 * want < p0[k].std() < 1.7 * want, (k, p0[k].std(), want)


def test_hidden_dropout_with_the_branch(hip_lib):
    """dnn_cate with dropout after both hidden layers (the tower input kept): five lazy steps
    against the restatement fed the masks of the header's words (tests/_dropout_ref.py)."""
    name, seed, keeps = "dnn_cate", 77, [1.0, 0.8, 0.7]
    _, P0 = _init(name, 0, 4)
    bs = _batches(name, 5, seed=21)
    dims = KW[name]["hidden"]

    def per_step(i, b):
        masks = [None] + [D.keep_mask(seed, i + 1, l + 1, B_, d, keeps[l + 1]) for l, d in enumerate(dims)]
        return dict(masks=masks, invs=[None] + [D.inv_keep(k) for k in keeps[1:]])
    zs, losses, P = _ref_run(name, P0, bs, per_step=per_step)
    eng = CTREngine(ModelSpec(name, afm_attention=AT, dropout_keep_deep=keeps, **KW[name]), max_batch=B_, init="none",
                    adam="lazy", seed=seed)
    eng.load_params({k: v.copy() for k, v in P0.items()})
    gz, gl = _run(eng, bs)
    _check(eng, gz, gl, zs, losses, P, "dropout")


def test_sample_weights_with_the_branch(hip_lib):
    """dnn_pipeline with sample_weight=True and pos_weight 2.5 (weights in {0, 0.5, 1, 3}): five lazy
    steps against the restatement's weighted loss."""
    name, pw = "dnn_pipeline", 2.5
    _, P0 = _init(name, 0, 6)
    bs = _batches(name, 5, seed=31)
    for i, b in enumerate(bs):
        b["weight"] = np.random.default_rng(90 + i).choice(np.float32([0, 0.5, 1, 3]), B_).reshape(B_, 1)
    per_step = lambda i, b: dict(w=W.w_eff_f32(b["weight"], b["label"], pw)[0])
    zs, losses, P = _ref_run(name, P0, bs, per_step=per_step)
    eng = CTREngine(ModelSpec(name, afm_attention=AT, pos_weight=pw, **KW[name]), max_batch=B_, init="none",
                    adam="lazy", sample_weight=True)
    eng.load_params({k: v.copy() for k, v in P0.items()})
    gz, gl = _run(eng, bs)
    _check(eng, gz, gl, zs, losses, P, "weighted")


# --------------------------------------------------------------------------- 3. predict and persistence
def test_predict_on_planes_equals_the_record_path(hip_lib):
    """Lazy tables: predict right after training, after flush() and after flush(planes=True) (the
    plane lookup, unfused because the branch reads x0) give the same bits, and they are the
    restatement's logits within 1e-5."""
    name = "dnn_pipeline"
    eng = CTREngine(ModelSpec(name, afm_attention=AT, **KW[name]), max_batch=B_, seed=9, adam="lazy")
    bs = _batches(name, 6, seed=40)
    for b in bs[:3]:
        eng.train_step(b, graph=True)
    torch.cuda.synchronize()
    assert eng.fused_gather_rows() and not eng.fused_gather_l0()
    b = bs[-1]
    z0 = eng.predict(b, logits=True)
    eng.flat_planes = False
    eng.flush()
    z1 = eng.predict(b, logits=True)
    eng.flat_planes = True
    eng.flush(planes=True)
    assert eng.planes_step == eng.steps and not eng.fused_gather_l0()
    z2 = eng.predict(b, logits=True)
    np.testing.assert_array_equal(z0, z1)
    np.testing.assert_array_equal(z0, z2)
    ref = Af.forward_backward(R.make_cfg(name, **KW[name]), eng.params(), b, 0, AT)
    assert np.abs(z0 - ref["z"]).max() < TOL


def test_checkpoint_and_export_round_trip(hip_lib, tmp_path):
    """A checkpoint saved after three steps and restored into a fresh model continues the
    trajectory bit for bit (logits of two more steps, every parameter, the attention moments); the
    exported model loads with its afm_attention and scores identically."""
    import types
    from deep_learning_amd.models._ctr_model import export_model, load_model
    from deep_learning_amd.models.dnn_pipeline import DeepModel
    kw = KW["dnn_pipeline"]
    args = types.SimpleNamespace(epochs=1, batch_size=B_, model_pb=str(tmp_path / "pb"),
                                 save_model_checkpoint=str(tmp_path / "ck"), model_restore=0,
                                 restore_model_checkpoint=str(tmp_path / "ck"), embedding_size=kw["E"],
                                 cate_feats_size=kw["cate_index_size"], hidden_units=kw["hidden"], learning_rate=1e-3,
                                 l2_reg=1e-5, learning_rate_decay_steps=1000, learning_rate_decay_rate=0.9,
                                 cate_field_size=kw["S"], cont_field_size=kw["C"], vector_feats_size=kw["V"],
                                 afm_attention=AT)
    bs = _batches("dnn_pipeline", 5, seed=60)
    a = DeepModel(args, bs)
    a.model_optimizer()
    assert a.engine.afm == AT
    for b in bs[:3]:
        a.engine.train_step(b, graph=True)
    a._save_checkpoint(args.save_model_checkpoint)
    r = DeepModel(args, bs)
    r.model_optimizer()
    r._restore(args.restore_model_checkpoint)
    for m in (a, r):
        m.zs = []
        for b in bs[3:]:
            m.engine.train_step(b, graph=True)
            torch.cuda.synchronize()
            m.zs.append(m.engine.z[:B_].cpu().numpy().copy())
    for x, y in zip(a.zs, r.zs):
        np.testing.assert_array_equal(x, y)
    pa, pr = a.engine.params(), r.engine.params()
    for k in pa:
        np.testing.assert_array_equal(pa[k], pr[k], err_msg=k)
    sa, sr = a.engine.dense_state(), r.engine.dense_state()
    for k in Af.AFM_KEYS:
        np.testing.assert_array_equal(sa["v"][k], sr["v"][k], err_msg=k)
        np.testing.assert_array_equal(sa["m"][k], sr["m"][k], err_msg=k)
    export_model(a.engine, args.model_pb)
    loaded = load_model(args.model_pb)
    assert loaded.spec.afm_attention == AT and loaded.afm == AT
    np.testing.assert_array_equal(loaded.predict(bs[0]), a.engine.predict(bs[0]))


def test_local_run_train_then_predict(hip_lib, tmp_path):
    """local_run.py dnn_pipeline ... afm_attention=4: train -> export -> predict end to end; the
    exported variables hold the attention variables and the printed AUC is the restatement's on them
    within 1e-4."""
    from deep_learning_amd.synthetic import make_batch
    from deep_learning_amd.utils import data_loader
    conf, tr, pr = tmp_path / "conf", tmp_path / "train", tmp_path / "pred"
    for p in (conf, tr, pr):
        p.mkdir()
    lines = ["f%d\tx\tfloat" % i for i in range(13)] + ["c%d\tx\tstring" % i for i in range(26)]
    (conf / "dnn.conf").write_text("\n".join(lines) + "\n")
    V = 3000
    for i in range(3):
        data_loader.write_tfrecord_part(str(tr / ("part-%d" % i)), make_batch(256, cate_index_size=V, seed=i))
    pred_part = make_batch(200, cate_index_size=V, seed=99)
    data_loader.write_tfrecord_part(str(pr / "part-0"), pred_part)
    args = ["dnn_pipeline", "train", "1", "8", str(V), "3", str(conf), str(tr) + "/", str(pr) + "/",
            str(tmp_path / "model_pb"), str(tmp_path / "ckpt"), "0", str(tmp_path / "ckpt"),
            "batch_size=64", "hidden_units=32,16", "shuffle=0", "afm_attention=4"]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "local_run.py")] + args, capture_output=True, text=True,
                       timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "afm_attention = 4" in r.stdout
    auc_gpu = float(r.stdout.split("val of auc:")[-1].split()[0])
    d = np.load(tmp_path / "model_pb" / "variables.npz")
    P = {k: d[k] for k in d.files}
    assert set(Af.AFM_KEYS) <= set(P) and P["attention_w"].shape == (8, 4) and P["attention_p"].shape == (8, 1)
    kw = dict(C=13, V=0, S=26, E=8, cate_index_size=V, hidden=[32, 16])
    b = {k: v[:192] for k, v in pred_part.items()}
    ref = Af.forward_backward(R.make_cfg("dnn_pipeline", **kw), P, b, 0, 4)
    assert abs(R.auc(b["label"], ref["p"]) - auc_gpu) < 1e-4


# --------------------------------------------------------------------------- 4. the default
@pytest.mark.parametrize("adam", ["dense", "lazy"])
def test_default_queues_the_kernels_it_queued(hip_lib, adam, monkeypatch):
    """afm_attention = 0: a step's and a predict's entry-point sequence equals that of an engine
    built without the argument, and holds none of the new entry points or buffers; with
    afm_attention = 4 the same sequence plus the new launches."""
    from deep_learning_amd import engine as E
    names = []
    real = E.call
    monkeypatch.setattr(E, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    name = "dnn_pipeline"
    bs = _batches(name, 2, seed=70)
    seqs = []
    for extra in ({}, {"afm_attention": 0}, {"afm_attention": AT}):
        eng = CTREngine(ModelSpec(name, **extra, **KW[name]), max_batch=B_, seed=3, adam=adam)
        del names[:]
        eng.train_step(bs[0])
        eng.predict(bs[1])
        torch.cuda.synchronize()
        seqs.append(list(names))
        if not extra.get("afm_attention"):
            assert "afm" not in eng.groups and not any(hasattr(eng, a) for a in ("z_afm", "afm_stats"))
    assert seqs[0] == seqs[1] and len(seqs[0]) > 8
    assert not any("afm" in n or "cross" in n for n in seqs[0])
    new = ["dl_afm_fwd", "dl_head_fwd_bwd_cross", "dl_afm_bwd", "dl_adam_dense"]
    rest = list(seqs[2])
    for n in new + ["dl_afm_fwd", "dl_head_fwd_bwd_cross"]:      # the step's four, predict's two
        rest.remove(n)
    assert rest == [n for n in seqs[0] if n != "dl_head_fwd_bwd"]
    assert seqs[0].count("dl_head_fwd_bwd") == 2
