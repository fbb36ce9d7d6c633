"""GPU checks of the inner-product layer (ModelSpec.pnn, csrc/pnn.hip):
dl_pnn_inner_fwd / dl_pnn_inner_bwd against the float64 formulas (tests/_pnn_ref.py); five-step
trajectories of the four dnn_* models against the float64 restatement in every table mode, with the
cross network and the attention, with later-layer dropout, with sample weights and with one hidden
layer; predict, checkpoint, export and local_run; and the unchanged kernel sequence at pnn = None.

Kernel shapes (F, E, D1): (2, 8, 1) the smallest, two samples a tile; (3, 16, 33) odd F, a partial
third column tile; (26, 16, 50) and (26, 16, 400) the flagship's fields, fewer and more column tiles
than backward waves; (33, 8, 416) three field tiles, theta split into two D1-chunks in the backward;
(64, 32, 48) the largest F and E, two tiles a sample, four backward waves; B = 1, 63, 300 (a
partial last unit, more than one pass of the backward's capped grid)."""
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
from tests import _dropout_ref as D
from tests import _pnn_ref as Pn
from tests import _sample_weight_ref as W

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-5          # tests/test_gpu_parity.py: absolute, on logits and dense gradients / parameters
KW = {"dnn_pipeline": dict(C=13, V=3, S=8, E=8, cate_index_size=1000, hidden=[32, 16]),
      "dnn_cate": dict(V=2, S=8, E=8, cate_index_size=1000, hidden=[32, 16]),
      "dnn_multi": dict(C=5, V=2, S=4, E=8, cate_index_size=1000, hidden=[32, 16],
                        multi_ranges=[[0, 7, "a"], [7, 12, "b"]]),
      "dnn_multi_cate": dict(V=0, S=4, E=8, cate_index_size=1000, hidden=[32, 16],
                             multi_ranges=[[0, 5, "a"], [5, 6, "b"]])}
MODES = {"atomic": dict(bwd="atomic"), "sorted": dict(bwd="sorted"), "lazy": dict(adam="lazy")}
B_ = 64
SHAPES = [(2, 8, 1), (3, 16, 33), (26, 16, 50), (26, 16, 400), (33, 8, 416), (64, 32, 48)]
THETA_SCALE = 0.3   # injected theta: lp ~ 1e-2, so the layer moves the logits far beyond the tolerance
X_COL0, DX_COL0 = 3, 2


def _s():
    return _lib.stream_handle()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


# --------------------------------------------------------------------------- 1. the kernels
def _run_kernels(fx, runs=1, with_bits=True):
    """dl_pnn_inner_fwd then dl_pnn_inner_bwd on a fixture: x0 [B, 3 + F E + 5] (pads 7.0, never read,
    the fields from column 3), C [B + 1, D1 + 3], d with its own pitch, dx0 pre-filled, the fields from
    its column 2 and 3 more columns after them.  Returns per run (C, bits, dx, slab)."""
    x, theta, c, d, _ = fx
    B, F, E = x.shape
    D1 = theta.shape[0]
    ld = X_COL0 + F * E + 5
    x0 = np.full((B, ld), 7.0, np.float32)
    x0[:, X_COL0:X_COL0 + F * E] = x.reshape(B, F * E)
    ldc, ldd, ldb = D1 + 3, D1 + 1, (D1 + 15) // 16 + 2
    c0 = np.full((B + 1, ldc), -7.0, np.float32)
    c0[:B, :D1] = c
    dd = np.full((B, ldd), 9.0, np.float32)
    dd[:, :D1] = d
    dx_ld = DX_COL0 + F * E + 3
    pre = (np.random.default_rng(5).standard_normal((B, dx_ld)) * 0.1).astype(np.float32)
    dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in dict(x0=x0, th=theta, d=dd).items()}
    grid = _lib.lib().dl_pnn_grid(B)
    outs = []
    for _ in range(runs):
        C = torch.from_numpy(c0).cuda()
        bits = torch.full((B + 1, ldb), 0x5555, dtype=torch.int16, device="cuda")
        dx = torch.from_numpy(pre).cuda()
        slab = torch.full((grid + 1, D1 * F), -7.0, device="cuda")
        call("dl_pnn_inner_fwd", B, F, E, D1, ptr(dev["x0"]), ld, X_COL0, ptr(dev["th"]), ptr(C), ldc,
             ptr(bits) if with_bits else None, ldb if with_bits else 0, _s())
        call("dl_pnn_inner_bwd", B, F, E, D1, ptr(dev["x0"]), ld, X_COL0, ptr(dev["th"]), ptr(dev["d"]), ldd, ptr(dx),
             dx_ld, DX_COL0, ptr(slab), grid, _s())
        torch.cuda.synchronize()
        outs.append(tuple(t.cpu().numpy() for t in (C, bits, dx, slab)))
    return outs, c0, pre, grid


@pytest.mark.parametrize("B", [1, 63, 300])
@pytest.mark.parametrize("F,E,D1", SHAPES)
def test_pnn_kernels_match_fp64(hip_lib, F, E, D1, B):
    """h0 = relu(c + lp), dx0's addend and the slab's column sums (dtheta) within 1e-5 (absolute) of
    the float64 formulas; every non-padding lp >= 1e-2 (T / lp well conditioned), the all-padding
    sample has lp = 0 and adds nothing; the sign bits equal the reference's wherever its
    |pre-activation| > 1e-4 (at most 1 % left out, asserted on the reference), zero bits past D1, the
    halfwords past the row's and the pad columns of C untouched; dx0's other columns keep their bits;
    two runs give the same bits; without a bitmask C is the same.  Measured worst errors: DESIGN 4m."""
    fx = Pn.kernel_fixture(B, F, E, D1, seed=1000 * F + D1 + B)
    x, theta, c, d, pad = fx
    lp64, _ = Pn.pnn_fwd64(x, theta)
    live = np.ones(B, bool)
    if pad is not None:
        live[pad] = False
        assert (lp64[pad] == 0).all()
    assert lp64[live].min() >= 1e-2
    pre64 = c.astype(np.float64) + lp64
    sure = np.abs(pre64) > 1e-4
    assert sure.mean() >= 0.99
    assert B * D1 < 100 or 0.05 < (pre64 > 0).mean() < 0.95      # both signs occur
    ddx, dth = Pn.pnn_bwd64(x, theta, d)
    outs, c0, pre, grid = _run_kernels(fx, runs=2)
    assert 1 <= grid <= 512 and _lib.lib().dl_pnn_grid(1 << 20) == 512
    for a, b in zip(outs[0], outs[1]):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    Cg, bg, dxg, slg = outs[0]
    assert np.array_equal(_bits(Cg[B]), _bits(c0[B])) and np.array_equal(_bits(Cg[:, D1:]), _bits(c0[:, D1:]))
    assert (slg[grid] == -7).all()
    nh = (D1 + 15) // 16
    assert (bg[B] == 0x5555).all() and (bg[:, nh:] == 0x5555).all()
    got_bits = ((bg[:B, :nh].astype(np.int32)[:, :, None] >> np.arange(16)) & 1).reshape(B, nh * 16)
    assert (got_bits[:, D1:] == 0).all()
    assert np.array_equal(got_bits[:, :D1][sure], (pre64 > 0)[sure].astype(np.int32))
    assert np.array_equal(got_bits[:, :D1] == 1, Cg[:B, :D1] > 0)
    lo, hi = DX_COL0, DX_COL0 + F * E
    assert np.array_equal(_bits(dxg[:, :lo]), _bits(pre[:, :lo])) and np.array_equal(_bits(dxg[:, hi:]), _bits(pre[:, hi:]))
    if pad is not None:
        assert np.array_equal(_bits(dxg[pad]), _bits(pre[pad]))
    assert np.abs(ddx).max() > 0 and np.abs(dth).max() > 0
    err = dict(h0=np.abs(Cg[:B, :D1] - np.maximum(pre64, 0)).max(),
               dx0=np.abs(dxg[:, lo:hi] - (pre[:, lo:hi].astype(np.float64) + ddx.reshape(B, F * E))).max(),
               slab=np.abs(slg[:grid].astype(np.float64).sum(0) - dth.reshape(-1)).max())
    print("max |kernel - fp64|:", {k: float(v) for k, v in err.items()})
    for k, v in err.items():
        assert v < TOL, (k, v)
    (nobits,), _, _, _ = _run_kernels(fx, with_bits=False)
    assert np.array_equal(_bits(nobits[0]), _bits(Cg)) and (nobits[1] == 0x5555).all()


def test_pnn_kernels_refuse_what_they_cannot_take(hip_lib):
    t = torch.full((8, 2200), 3.0, device="cuda")
    th = torch.zeros(4096, device="cuda")
    out = torch.full((8, 64), 3.0, device="cuda")
    slab = torch.full((4096,), 3.0, device="cuda")
    bits = torch.full((8, 8), 3, dtype=torch.int16, device="cuda")
    for F, E, D1 in ((1, 8, 4), (65, 8, 4), (4, 12, 4), (4, 8, 0)):
        with pytest.raises(_lib.DLError, match="F %d fields|E %d not|D1 %d < 1" % (F, E, D1)):
            call("dl_pnn_inner_fwd", 8, F, E, D1, ptr(t), 2200, 0, ptr(th), ptr(out), 64, ptr(bits), 8, _s())
        with pytest.raises(_lib.DLError, match="F %d fields|E %d not|D1 %d < 1" % (F, E, D1)):
            call("dl_pnn_inner_bwd", 8, F, E, D1, ptr(t), 2200, 0, ptr(th), ptr(out), 64, ptr(t), 2200, 0, ptr(slab), 1,
                 _s())
    with pytest.raises(_lib.DLError, match="field columns"):     # fields past x0's row
        call("dl_pnn_inner_fwd", 8, 4, 8, 4, ptr(t), 2200, 2190, ptr(th), ptr(out), 64, None, 0, _s())
    with pytest.raises(_lib.DLError, match="ldc"):
        call("dl_pnn_inner_fwd", 8, 4, 8, 4, ptr(t), 2200, 0, ptr(th), ptr(out), 3, None, 0, _s())
    with pytest.raises(_lib.DLError, match="ldbits"):
        call("dl_pnn_inner_fwd", 8, 4, 8, 40, ptr(t), 2200, 0, ptr(th), ptr(out), 64, ptr(bits), 2, _s())
    with pytest.raises(_lib.DLError, match="dx0 columns"):
        call("dl_pnn_inner_bwd", 8, 4, 8, 4, ptr(t), 2200, 0, ptr(th), ptr(out), 64, ptr(t), 2200, 2190, ptr(slab), 1, _s())
    with pytest.raises(_lib.DLError, match="slab needs"):
        call("dl_pnn_inner_bwd", 64, 4, 8, 4, ptr(t), 2200, 0, ptr(th), ptr(out), 64, ptr(t), 2200, 0, ptr(slab), 1, _s())
    torch.cuda.synchronize()
    assert (t == 3).all() and (out == 3).all() and (slab == 3).all() and (bits == 3).all()


# --------------------------------------------------------------------------- 2. the engine
def _batches(name, n, seed=11, B=B_, kw=None):
    return [Pn.X.make_batch(name, kw or KW[name], B, seed + i) for i in range(n)]


def _init(name, seed, L=0, A=0, kw=None):
    """Injected parameters at the models' init scales, theta at THETA_SCALE."""
    cfg = R.make_cfg(name, **(kw or KW[name]))
    return cfg, Pn.init_params(cfg, L, A, True, np.random.default_rng(seed), scale=THETA_SCALE)


def _ref_run(name, P0, bs, L=0, A=0, kw=None, **opts):
    cfg = R.make_cfg(name, **(kw or KW[name]))
    P = {k: v.copy() for k, v in P0.items()}
    opt = R.AdamTF1(cfg, P)
    zs, losses = [], []
    for i, b in enumerate(bs):
        fw = Pn.train_step(cfg, P, opt, b, L, A, True, **(opts["per_step"](i, b) if "per_step" in opts else {}))
        zs.append(fw["z"])
        losses.append(fw["loss"])
    return zs, losses, P


@pytest.fixture(scope="module")
def trajectories():
    """The restatement's five steps from injected parameters, once per model."""
    out = {}
    for name in KW:
        _, P0 = _init(name, 42)
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
    assert got[Pn.KEY].shape == P[Pn.KEY].shape
    err["params"] = max(np.abs(got[k] - P[k]).max() for k in P)
    err["theta"] = np.abs(got[Pn.KEY] - P[Pn.KEY]).max()
    print(tag, "max |engine - restatement|:", {k: float(v) for k, v in err.items()})
    for k, v in err.items():
        assert v < TOL, (k, v)
    return got


@pytest.mark.parametrize("name", list(KW))
def test_trajectory_matches_restatement(hip_lib, trajectories, name):
    """Five steps (two eager, three replayed as a hipGraph) in every table mode: each step's logits
    and loss and the final parameters (theta among them) within 1e-5 of the restatement; lazy and
    sorted + dense bit for bit (dnn_pipeline, dnn_cate: the multi-hot models' dense pooled scatter is
    atomic)."""
    P0, bs, zs, losses, P = trajectories[name]
    res = {}
    for mode, ekw in MODES.items():
        eng = CTREngine(ModelSpec(name, pnn="inner", **KW[name]), max_batch=B_, init="none", **ekw)
        eng.load_params({k: v.copy() for k, v in P0.items()})
        gz, gl = _run(eng, bs)
        res[mode] = (gz, _check(eng, gz, gl, zs, losses, P, "%s %s" % (name, mode)), eng.dense_state())
    for mv in ("m", "v"):
        assert np.abs(res["lazy"][2][mv][Pn.KEY]).max() > 0
    if "multi_ranges" not in KW[name]:
        for a, b in zip(res["lazy"][0], res["sorted"][0]):
            np.testing.assert_array_equal(a, b)
        for k in res["lazy"][1]:
            np.testing.assert_array_equal(res["lazy"][1][k], res["sorted"][1][k], err_msg=k)
        for mv in ("m", "v"):
            np.testing.assert_array_equal(res["lazy"][2][mv][Pn.KEY], res["sorted"][2][mv][Pn.KEY])
    # the layer does matter: the same steps without it end elsewhere
    plain = CTREngine(ModelSpec(name, **KW[name]), max_batch=B_, init="none", adam="lazy")
    plain.load_params({k: v.copy() for k, v in P0.items() if k != Pn.KEY})
    plain.train_step(bs[0])
    torch.cuda.synchronize()
    assert np.abs(plain.z[:B_].cpu().numpy() - zs[0]).max() > 5 * TOL
    assert np.abs(P[Pn.KEY] - P0[Pn.KEY]).max() > 100 * TOL


def test_with_the_cross_network_and_the_attention(hip_lib):
    """dnn_multi with cross_layers = 2 and afm_attention = 4 as well."""
    name = "dnn_multi"
    _, P0 = _init(name, 43, L=2, A=4)
    bs = _batches(name, 5, seed=15)
    zs, losses, P = _ref_run(name, P0, bs, L=2, A=4)
    eng = CTREngine(ModelSpec(name, pnn="inner", afm_attention=4, cross_layers=2, **KW[name]), max_batch=B_,
                    init="none", adam="lazy")
    eng.load_params({k: v.copy() for k, v in P0.items()})
    gz, gl = _run(eng, bs)
    _check(eng, gz, gl, zs, losses, P, "cross + afm + pnn")


def test_one_hidden_layer_has_no_sign_bitmask(hip_lib):
    """hidden = [24]: the head masks dh[0] by h[0] > 0 itself; dense and lazy."""
    name = "dnn_pipeline"
    kw = dict(KW[name], hidden=[24])
    _, P0 = _init(name, 44, kw=kw)
    bs = _batches(name, 5, seed=17, kw=kw)
    zs, losses, P = _ref_run(name, P0, bs, kw=kw)
    for mode in ("atomic", "lazy"):
        eng = CTREngine(ModelSpec(name, pnn="inner", **kw), max_batch=B_, init="none", **MODES[mode])
        assert len(eng.hbits) == 0
        eng.load_params({k: v.copy() for k, v in P0.items()})
        gz, gl = _run(eng, bs)
        _check(eng, gz, gl, zs, losses, P, "one layer %s" % mode)


def test_same_seed_runs_agree_bit_for_bit(hip_lib):
    """Device-initialised engines of one seed, five graph steps each: logits, every parameter and
    theta's moments equal bit for bit; theta is drawn at the reference's scale and shape."""
    name = "dnn_multi"
    bs = _batches(name, 5, seed=3)
    out = []
    for _ in range(2):
        eng = CTREngine(ModelSpec(name, pnn="inner", **KW[name]), max_batch=B_, seed=7, adam="lazy")
        p0 = eng.params()
        zs, _ = _run(eng, bs, graph_from=0)
        out.append((zs, eng.params(), eng.dense_state(), p0))
    for a, b in zip(out[0][0], out[1][0]):
        np.testing.assert_array_equal(a, b)
    for k in out[0][1]:
        np.testing.assert_array_equal(out[0][1][k], out[1][1][k], err_msg=k)
    np.testing.assert_array_equal(out[0][2]["v"][Pn.KEY], out[1][2]["v"][Pn.KEY])
    th = out[0][3][Pn.KEY]
    assert th.shape == (32, 6) and 0.005 < th.std() < 0.017


def test_later_layer_dropout_with_the_layer(hip_lib):
    """dnn_cate with dropout after the second hidden layer (the tower input and the first layer
    kept): five lazy steps against the restatement fed the masks of the header's words
    (tests/_dropout_ref.py)."""
    name, seed, keeps = "dnn_cate", 77, [1.0, 1.0, 0.7]
    _, P0 = _init(name, 4)
    bs = _batches(name, 5, seed=21)
    dims = KW[name]["hidden"]

    def per_step(i, b):
        masks = [None, None, D.keep_mask(seed, i + 1, 2, B_, dims[1], keeps[2])]
        return dict(masks=masks, invs=[None, None, D.inv_keep(keeps[2])])
    zs, losses, P = _ref_run(name, P0, bs, per_step=per_step)
    eng = CTREngine(ModelSpec(name, pnn="inner", dropout_keep_deep=keeps, **KW[name]), max_batch=B_, init="none",
                    adam="lazy", seed=seed)
    eng.load_params({k: v.copy() for k, v in P0.items()})
    gz, gl = _run(eng, bs)
    _check(eng, gz, gl, zs, losses, P, "dropout")


def test_sample_weights_with_the_layer(hip_lib):
    """dnn_pipeline with sample_weight=True and pos_weight 2.5 (weights in {0, 0.5, 1, 3}): five lazy
    steps against the restatement's weighted loss."""
    name, pw = "dnn_pipeline", 2.5
    _, P0 = _init(name, 6)
    bs = _batches(name, 5, seed=31)
    for i, b in enumerate(bs):
        b["weight"] = np.random.default_rng(90 + i).choice(np.float32([0, 0.5, 1, 3]), B_).reshape(B_, 1)
    per_step = lambda i, b: dict(w=W.w_eff_f32(b["weight"], b["label"], pw)[0])
    zs, losses, P = _ref_run(name, P0, bs, per_step=per_step)
    eng = CTREngine(ModelSpec(name, pnn="inner", pos_weight=pw, **KW[name]), max_batch=B_, init="none",
                    adam="lazy", sample_weight=True)
    eng.load_params({k: v.copy() for k, v in P0.items()})
    gz, gl = _run(eng, bs)
    _check(eng, gz, gl, zs, losses, P, "weighted")


# --------------------------------------------------------------------------- 3. predict and persistence
def test_predict_on_planes_equals_the_record_path(hip_lib):
    """Lazy tables: predict right after training, after flush() and after flush(planes=True) (the
    plane lookup, unfused because the layer reads x0) give the same bits, and they are the
    restatement's logits within 1e-5."""
    name = "dnn_pipeline"
    eng = CTREngine(ModelSpec(name, pnn="inner", **KW[name]), max_batch=B_, init="none", adam="lazy")
    _, P0 = _init(name, 9)
    eng.load_params(P0)
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
    ref = Pn.forward_backward(R.make_cfg(name, **KW[name]), eng.params(), b, pnn=True)
    assert np.abs(z0 - ref["z"]).max() < TOL


def test_checkpoint_and_export_round_trip(hip_lib, tmp_path):
    """A checkpoint saved after three steps and restored into a fresh model continues the
    trajectory bit for bit (logits of two more steps, every parameter, theta's moments); the exported
    model loads with its pnn and scores identically."""
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
                                 pnn="inner")
    bs = _batches("dnn_pipeline", 5, seed=60)
    a = DeepModel(args, bs)
    a.model_optimizer()
    assert a.engine.pnn == "inner"
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
    for mv in ("m", "v"):
        assert np.abs(sa[mv][Pn.KEY]).max() > 0
        np.testing.assert_array_equal(sa[mv][Pn.KEY], sr[mv][Pn.KEY])
    export_model(a.engine, args.model_pb)
    loaded = load_model(args.model_pb)
    assert loaded.spec.pnn == "inner" and loaded.pnn == "inner"
    np.testing.assert_array_equal(loaded.predict(bs[0]), a.engine.predict(bs[0]))


def test_local_run_train_then_predict(hip_lib, tmp_path):
    """local_run.py dnn_pipeline ... pnn=inner: train -> export -> predict end to end; the exported
    variables hold theta and the printed AUC is the restatement's on them within 1e-4."""
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
            "batch_size=64", "hidden_units=32,16", "shuffle=0", "pnn=inner"]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "local_run.py")] + args, capture_output=True, text=True,
                       timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    auc_gpu = float(r.stdout.split("val of auc:")[-1].split()[0])
    d = np.load(tmp_path / "model_pb" / "variables.npz")
    P = {k: d[k] for k in d.files}
    assert P[Pn.KEY].shape == (32, 26)
    kw = dict(C=13, V=0, S=26, E=8, cate_index_size=V, hidden=[32, 16])
    b = {k: v[:192] for k, v in pred_part.items()}
    ref = Pn.forward_backward(R.make_cfg("dnn_pipeline", **kw), P, b, pnn=True)
    assert abs(R.auc(b["label"], ref["p"]) - auc_gpu) < 1e-4


# --------------------------------------------------------------------------- 4. the default
@pytest.mark.parametrize("adam", ["dense", "lazy"])
def test_default_queues_the_kernels_it_queued(hip_lib, adam, monkeypatch):
    """pnn = None: a step's and a predict's entry-point sequence equals that of an engine built
    without the argument, and holds none of the new entry points or buffers; with pnn = "inner" the
    same sequence plus the new launches."""
    from deep_learning_amd import engine as E
    names = []
    real = E.call
    monkeypatch.setattr(E, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    name = "dnn_pipeline"
    bs = _batches(name, 2, seed=70)
    seqs = []
    for extra in ({}, {"pnn": None}, {"pnn": "inner"}):
        eng = CTREngine(ModelSpec(name, **extra, **KW[name]), max_batch=B_, seed=3, adam=adam)
        del names[:]
        eng.train_step(bs[0])
        eng.predict(bs[1])
        torch.cuda.synchronize()
        seqs.append(list(names))
        if not extra.get("pnn"):
            assert "pnn" not in eng.groups
    assert seqs[0] == seqs[1] and len(seqs[0]) > 8
    assert not any("pnn" in n for n in seqs[0])
    rest = list(seqs[2])
    for n in ["dl_pnn_inner_fwd", "dl_pnn_inner_bwd", "dl_adam_dense", "dl_pnn_inner_fwd"]:   # the step's three, predict's one
        rest.remove(n)
    assert rest == seqs[0]
