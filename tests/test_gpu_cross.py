"""GPU checks of the cross network (ModelSpec.cross_layers, csrc/cross.hip):
dl_cross_fwd / dl_cross_bwd against the float64 formulas (tests/_cross_ref.py); the head's
z_extra twins; five-step trajectories of the four dnn_* models against the float64 restatement
in every table mode, with hidden-layer dropout and with sample weights; predict, checkpoint,
export and local_run; and the unchanged kernel sequence at cross_layers = 0.

Kernel shapes: D = 37 (below a wave), 64 (one wave), 221 / 429 / 525 (ragged, 4 / 8 / 16 values
a lane with a partial last one), 1024 (the most); L = 1, 2, 4 (every register variant);
B = 1, 63 (a partial block), 300 (19 blocks of four waves: four passes of the grid)."""
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
from tests import _cross_ref as X
from tests import _dropout_ref as D
from tests import _sample_weight_ref as W

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-5          # tests/test_gpu_parity.py: absolute, on logits and dense gradients / parameters
LC = 2
KW = {"dnn_pipeline": dict(C=13, V=3, S=8, E=8, cate_index_size=1000, hidden=[32, 16]),
      "dnn_cate": dict(V=2, S=8, E=8, cate_index_size=1000, hidden=[32, 16]),
      "dnn_multi": dict(C=5, V=2, S=4, E=8, cate_index_size=1000, hidden=[32, 16],
                        multi_ranges=[[0, 7, "a"], [7, 12, "b"]]),
      "dnn_multi_cate": dict(V=0, S=4, E=8, cate_index_size=1000, hidden=[32, 16],
                             multi_ranges=[[0, 5, "a"], [5, 6, "b"]])}
MODES = {"atomic": dict(bwd="atomic"), "sorted": dict(bwd="sorted"), "lazy": dict(adam="lazy")}
B_ = 64


def _s():
    return _lib.stream_handle()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


# --------------------------------------------------------------------------- 1. the kernels
def _cross_inputs(B, Dn, L, seed):
    """x0 and parameters at the engine's init scales: embedding columns ~ N(0, 0.01), the last
    (up to 13) columns dense features in [0, 1); w, b ~ N(0, sqrt(2 / 2D)), c ~ N(0, sqrt(2 / (D + 33)));
    dz a log-loss logit gradient's size, (p - y) / B."""
    rng = np.random.default_rng(seed)
    ld = (Dn + 1 + 15) // 16 * 16
    x0 = np.full((B, ld), 7.0, np.float32)         # the pad columns must not be read
    x0[:, :Dn] = rng.standard_normal((B, Dn)) * 0.01
    nc = min(13, Dn // 2)
    x0[:, Dn - nc:Dn] = rng.random((B, nc))
    prm = (rng.standard_normal((2 * L + 1, Dn)) * np.sqrt(1.0 / Dn)).astype(np.float32)
    prm[0] = rng.standard_normal(Dn) * np.sqrt(2.0 / (Dn + 33))
    dz = ((rng.random(B) - (rng.random(B) < 0.3)) / B).astype(np.float32)
    return x0, prm, dz, nc


@pytest.mark.parametrize("B", [1, 63, 300])
@pytest.mark.parametrize("L", [1, 2, 4])
@pytest.mark.parametrize("Dn", [37, 64, 221, 429, 525, 1024])
def test_cross_kernels_match_fp64(hip_lib, Dn, L, B):
    """s, z_cross, the slab's column sums (dc, dw_l, db_l) and dx0 within 1e-5 (absolute) of the
    float64 formulas; dx0 covers a column sub-range of x0 (the engine's [0, D - dense), and one
    that starts at column 3), is pre-filled and added into, and nothing outside it is written;
    two runs give the same bits.  Measured worst over the 54 cases (printed): s 1.1e-7,
    z_cross 2.0e-7, dx0 3.7e-8, slab sums 5.6e-8."""
    x0, prm, dz, nc = _cross_inputs(B, Dn, L, 1000 * L + Dn + B)
    dev = {k: torch.from_numpy(v).cuda() for k, v in dict(x0=x0, prm=prm.reshape(-1), dz=dz).items()}
    s = torch.full((B + 1, L), -7.0, device="cuda")
    zc = torch.full((B + 1,), -7.0, device="cuda")
    call("dl_cross_fwd", B, Dn, L, ptr(dev["x0"]), x0.shape[1], ptr(dev["prm"]), ptr(s), ptr(zc), _s())
    c, w, b = prm[0], prm[1:1 + L], prm[1 + L:]
    s64, z64, _ = X.cross_fwd64(x0[:, :Dn], c, w, b)
    ddx, dc, dw, db = X.cross_bwd64(x0[:, :Dn], c, w, b, dz)
    torch.cuda.synchronize()
    sg, zg = s.cpu().numpy(), zc.cpu().numpy()
    assert (sg[B] == -7).all() and zg[B] == -7
    err = dict(s=np.abs(sg[:B] - s64).max(), z=np.abs(zg[:B] - z64).max())
    grid = hip_lib.dl_cross_grid(B)
    assert 1 <= grid <= 512 and hip_lib.dl_cross_grid(1 << 20) == 512
    n = (2 * L + 1) * Dn
    want = np.concatenate([dc, dw.reshape(-1), db.reshape(-1)])
    for col0 in (0, 3):
        cols = Dn - nc - col0
        dx_ld = (cols + 3) // 4 * 4 + 4
        pre = (np.random.default_rng(5).standard_normal((B, dx_ld)) * 1e-3).astype(np.float32)
        outs = []
        for _ in range(2):
            dx = torch.from_numpy(pre).cuda()
            slab = torch.full((grid + 1, n), -7.0, device="cuda")
            call("dl_cross_bwd", B, Dn, L, ptr(dev["x0"]), x0.shape[1], ptr(dev["prm"]), ptr(s), ptr(dev["dz"]),
                 ptr(dx), dx_ld, col0, cols, ptr(slab), grid, _s())
            torch.cuda.synchronize()
            outs.append((dx.cpu().numpy(), slab.cpu().numpy()))
        (dxg, slg), (dx2, sl2) = outs
        assert np.array_equal(_bits(dxg), _bits(dx2)) and np.array_equal(_bits(slg), _bits(sl2))
        assert (slg[grid] == -7).all()
        assert np.array_equal(_bits(dxg[:, cols:]), _bits(pre[:, cols:]))
        err["dx0"] = max(err.get("dx0", 0), np.abs(dxg[:, :cols] - (pre[:, :cols] + ddx[:, col0:col0 + cols])).max())
        err["slab"] = max(err.get("slab", 0), np.abs(slg[:grid].astype(np.float64).sum(0) - want).max())
        assert np.abs(ddx[:, col0:col0 + cols]).max() > 0
    print("max |kernel - fp64|:", {k: float(v) for k, v in err.items()})
    for k, v in err.items():
        assert v < TOL, (k, v)


def test_cross_kernels_refuse_what_they_cannot_take(hip_lib):
    t = torch.zeros(8, 1040, device="cuda")
    prm = torch.zeros(11 * 1040, device="cuda")
    out = torch.zeros(8 * 8, device="cuda")
    slab = torch.zeros(11 * 1040, device="cuda")
    for Dn, L in ((1025, 2), (64, 5), (64, 0), (0, 1)):
        with pytest.raises(_lib.DLError, match="D %d|cross layers %d" % (Dn, L)):
            call("dl_cross_fwd", 8, Dn, L, ptr(t), 1040, ptr(prm), ptr(out), ptr(out), _s())
        with pytest.raises(_lib.DLError, match="D %d|cross layers %d" % (Dn, L)):
            call("dl_cross_bwd", 8, Dn, L, ptr(t), 1040, ptr(prm), ptr(out), ptr(out), ptr(t), 1040, 0, 0,
                 ptr(slab), 1, _s())
    with pytest.raises(_lib.DLError, match="dx0 columns"):      # dx0 columns past x0's
        call("dl_cross_bwd", 8, 64, 2, ptr(t), 1040, ptr(prm), ptr(out), ptr(out), ptr(t), 1040, 60, 8, ptr(slab), 1,
             _s())
    with pytest.raises(_lib.DLError, match="slab needs"):
        call("dl_cross_bwd", 64, 64, 2, ptr(t), 1040, ptr(prm), ptr(out), ptr(out), ptr(t), 1040, 0, 8, ptr(slab), 1,
             _s())


# --------------------------------------------------------------------------- 2. the head
def _head(B, weighted, zx):
    """dl_head_fwd_bwd_cross[_weighted] (zx given) or the plain entry point (zx None)."""
    g = torch.Generator().manual_seed(31 + B)
    F, E, H = 5, 8, 32
    fm_cols, fm_ld, ldh = F + E, F + E + 3, H + 4
    fm = torch.randn(B, fm_ld, generator=g)
    h = torch.relu(torch.randn(B, ldh, generator=g))
    w = torch.randn(fm_cols + H + 1, generator=g) * 0.1
    y = (torch.rand(B, generator=g) < 0.3).float()
    we = torch.from_numpy(W.w_eff_f32(np.random.default_rng(B).choice(np.float32([0, 0.5, 1, 3]), B), y.numpy(),
                                      2.5)[0]) if weighted else torch.ones(B)
    nz = int(np.count_nonzero(we.numpy()))
    norm = torch.tensor([np.float32(1.0 / nz) if nz else 0.0, float(nz)], dtype=torch.float32).cuda()
    grid = _lib.lib().dl_head_grid(B)
    out = {k: v.cuda() for k, v in dict(score=torch.zeros(B), z=torch.zeros(B), dz=torch.zeros(B),
                                        dh=torch.zeros(B, ldh), slab=torch.zeros(grid, fm_cols + H + 2)).items()}
    dev = [t.cuda() for t in (fm, h, w, y, we)]
    scale = [ptr(dev[4]), ptr(norm)] if weighted else [float(np.float32(1.0 / B))]
    extra = [] if zx is None else [ptr(zx)]
    name = "dl_head_fwd_bwd" + ("" if zx is None else "_cross") + ("_weighted" if weighted else "")
    call(name, B, fm_cols, H, ptr(dev[0]), fm_ld, ptr(dev[1]), ldh, ptr(dev[2]), ptr(dev[3]), 1e-7, *scale, *extra,
         ptr(out["score"]), ptr(out["z"]), ptr(out["dz"]), ptr(out["dh"]), ptr(out["slab"]), grid, _s())
    torch.cuda.synchronize()
    feat = np.concatenate([fm[:, :fm_cols].numpy(), h[:, :H].numpy()], 1).astype(np.float64)
    return {k: v.cpu().numpy() for k, v in out.items()}, (feat, w.numpy(), y.numpy(), we.numpy(), H, fm_cols)


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("B", [1, 67, 300])
def test_head_with_extra_logit(hip_lib, B, weighted):
    """z_extra = 0: every output equals the plain entry point's, bit for bit.  A random z_extra:
    score, z, dz, dh and the slab against the float64 head on the shifted logit (z_extra as one
    more feature of weight 1), each within 1e-5 of the array's largest magnitude as the other
    heads' tests.  Measured worst over the six cases (printed): score 7.7e-8,
    z 6.9e-8, dz 1.6e-7, dh 1.9e-7, slab 1.7e-7, loss column 5.3e-8."""
    plain, _ = _head(B, weighted, None)
    zero, _ = _head(B, weighted, torch.zeros(B, device="cuda"))
    for k in plain:
        assert np.array_equal(_bits(plain[k]), _bits(zero[k])), k
    zx = torch.randn(B, generator=torch.Generator().manual_seed(B)) * 0.5
    got, (feat, w, y, we, H, fm_cols) = _head(B, weighted, zx.cuda())
    ref = W.head64(np.concatenate([feat, zx.numpy().astype(np.float64)[:, None]], 1), np.concatenate([w[:-1], [1.0]]),
                   float(w[-1]), y, we)
    rel = lambda a, r: float(np.abs(np.asarray(a, np.float64) - r).max() / max(np.abs(r).max(), 1e-30))
    slab = got["slab"].astype(np.float64).sum(0)
    lsum = float((we.astype(np.float64) * W.per_sample_loss(ref["p"], y, 1e-7)).sum())
    # z against the magnitude of what is summed (a lone logit can cancel to near 0, B = 1): the f32
    # sum of its 47 terms is within 47 * 2^-24 = 2.8e-6 of sum |term|, inside the project's 1e-5
    zmag = (np.abs(feat * w[None, :-1]).sum(1) + abs(float(w[-1])) + np.abs(zx.numpy())).max()
    err = dict(score=rel(got["score"], ref["p"]), z=float(np.abs(got["z"] - ref["z"]).max() / zmag),
               dz=rel(got["dz"], ref["dz"]),
               dh=rel(got["dh"][:, :H], ref["dfeat"][:, fm_cols:fm_cols + H] * (feat[:, fm_cols:] > 0)),
               slab=rel(slab[:-1], np.concatenate([ref["dw"][:-1], [ref["db"]]])),
               loss=abs(slab[-1] - lsum) / max(abs(lsum), 1e-30))
    print("max relative error:", err)
    for k, v in err.items():
        assert v < TOL, (k, v)
    assert np.abs(got["z"] - plain["z"]).max() > 1e-3


# --------------------------------------------------------------------------- 3. the engine
def _batches(name, n, seed=11, B=B_):
    return [X.make_batch(name, KW[name], B, seed + i) for i in range(n)]


def _ref_run(name, P0, bs, **kw):
    cfg = R.make_cfg(name, **KW[name])
    P = {k: v.copy() for k, v in P0.items()}
    opt = R.AdamTF1(cfg, P)
    zs, losses = [], []
    for i, b in enumerate(bs):
        fw = X.train_step(cfg, P, opt, b, LC, **(kw["per_step"](i, b) if "per_step" in kw else {}))
        zs.append(fw["z"])
        losses.append(fw["loss"])
    return zs, losses, P


@pytest.fixture(scope="module")
def trajectories():
    """The restatement's five steps from injected parameters, once per model."""
    out = {}
    for name in KW:
        cfg = R.make_cfg(name, **KW[name])
        P0 = X.init_params(cfg, LC, np.random.default_rng(42))
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
    err["params"] = max(np.abs(got[k] - P[k]).max() for k in P)
    print(tag, "max |engine - restatement|:", {k: float(v) for k, v in err.items()})
    for k, v in err.items():
        assert v < TOL, (k, v)
    return got


@pytest.mark.parametrize("name", list(KW))
def test_trajectory_matches_restatement(hip_lib, trajectories, name):
    """Five steps (two eager, three replayed as a hipGraph) in every table mode: each step's
    logits and loss and the final parameters (the cross vectors among them) within 1e-5 of the
    restatement; lazy and sorted + dense bit for bit (dnn_pipeline, dnn_cate: as without the
    cross, the multi-hot models' dense pooled scatter is atomic).  Measured worst over the four models, the
    three modes and the dropout / weighted runs below (printed): logits 2.4e-7, loss 1.7e-7,
    parameters 1.7e-7."""
    P0, bs, zs, losses, P = trajectories[name]
    res = {}
    for mode, ekw in MODES.items():
        eng = CTREngine(ModelSpec(name, cross_layers=LC, **KW[name]), max_batch=B_, init="none", **ekw)
        eng.load_params({k: v.copy() for k, v in P0.items()})
        gz, gl = _run(eng, bs)
        res[mode] = (gz, _check(eng, gz, gl, zs, losses, P, "%s %s" % (name, mode)), eng.dense_state())
    for mv in ("m", "v"):
        for k in X.cross_keys(LC):
            assert np.abs(res["lazy"][2][mv][k]).max() > 0
    # lazy against sorted + dense, bit for bit — where they are so without the cross: with multi-hot
    # slots the dense engine adds the pooled gradients with atomics, whose order varies
    # (tests/test_gpu_parity.py test_lazy_adam_bit_identical_to_dense leaves those models out)
    if "multi_ranges" not in KW[name]:
        for a, b in zip(res["lazy"][0], res["sorted"][0]):
            np.testing.assert_array_equal(a, b)
        for k in res["lazy"][1]:
            np.testing.assert_array_equal(res["lazy"][1][k], res["sorted"][1][k], err_msg=k)
        for mv in ("m", "v"):
            for k in X.cross_keys(LC):
                np.testing.assert_array_equal(res["lazy"][2][mv][k], res["sorted"][2][mv][k], err_msg=k)
    # the cross does matter: the same steps without it end elsewhere
    plain = CTREngine(ModelSpec(name, **KW[name]), max_batch=B_, init="none", adam="lazy")
    plain.load_params({k: v.copy() for k, v in P0.items() if not k.startswith("cross_")})
    plain.train_step(bs[0])
    torch.cuda.synchronize()
    assert np.abs(plain.z[:B_].cpu().numpy() - zs[0]).max() > 100 * TOL


def test_same_seed_runs_agree_bit_for_bit(hip_lib):
    """Device-initialised engines of one seed, five graph steps each: logits, every parameter and
    the cross moments equal bit for bit; the cross vectors are drawn at their reference scales."""
    name = "dnn_multi"
    bs = _batches(name, 5, seed=3)
    out = []
    for _ in range(2):
        eng = CTREngine(ModelSpec(name, cross_layers=LC, **KW[name]), max_batch=B_, seed=7, adam="lazy")
        p0 = eng.params()
        zs, _ = _run(eng, bs, graph_from=0)
        out.append((zs, eng.params(), eng.dense_state(), p0))
    for a, b in zip(out[0][0], out[1][0]):
        np.testing.assert_array_equal(a, b)
    for k in out[0][1]:
        np.testing.assert_array_equal(out[0][1][k], out[1][1][k], err_msg=k)
    for k in X.cross_keys(LC):
        np.testing.assert_array_equal(out[0][2]["v"][k], out[1][2]["v"][k], err_msg=k)
    Dn, H = eng.D0, KW[name]["hidden"][-1]
    p0 = out[0][3]
    for k in X.cross_keys(LC):
        want = np.sqrt(2.0 / (Dn + H + 1)) if k == "cross_res" else np.sqrt(1.0 / Dn)
        assert p0[k].shape == (Dn, 1) and 0.6 * want < p0[k].std() < 1.5 * want, (k, p0[k].std(), want)


def test_hidden_dropout_with_the_cross(hip_lib):
    """dnn_cate with dropout after both hidden layers (the tower input kept): five lazy steps
    against the restatement fed the masks of the header's words (tests/_dropout_ref.py)."""
    name, seed, keeps = "dnn_cate", 77, [1.0, 0.8, 0.7]
    cfg = R.make_cfg(name, **KW[name])
    P0 = X.init_params(cfg, LC, np.random.default_rng(4))
    bs = _batches(name, 5, seed=21)
    dims = KW[name]["hidden"]

    def per_step(i, b):
        masks = [None] + [D.keep_mask(seed, i + 1, l + 1, B_, d, keeps[l + 1]) for l, d in enumerate(dims)]
        return dict(masks=masks, invs=[None] + [D.inv_keep(k) for k in keeps[1:]])
    zs, losses, P = _ref_run(name, P0, bs, per_step=per_step)
    eng = CTREngine(ModelSpec(name, cross_layers=LC, dropout_keep_deep=keeps, **KW[name]), max_batch=B_, init="none",
                    adam="lazy", seed=seed)
    eng.load_params({k: v.copy() for k, v in P0.items()})
    gz, gl = _run(eng, bs)
    _check(eng, gz, gl, zs, losses, P, "dropout")


def test_sample_weights_with_the_cross(hip_lib):
    """dnn_pipeline with sample_weight=True and pos_weight 2.5 (weights in {0, 0.5, 1, 3}): five lazy
    steps against the restatement's weighted loss."""
    name, pw = "dnn_pipeline", 2.5
    cfg = R.make_cfg(name, **KW[name])
    P0 = X.init_params(cfg, LC, np.random.default_rng(6))
    bs = _batches(name, 5, seed=31)
    for i, b in enumerate(bs):
        b["weight"] = np.random.default_rng(90 + i).choice(np.float32([0, 0.5, 1, 3]), B_).reshape(B_, 1)
    per_step = lambda i, b: dict(w=W.w_eff_f32(b["weight"], b["label"], pw)[0])
    zs, losses, P = _ref_run(name, P0, bs, per_step=per_step)
    eng = CTREngine(ModelSpec(name, cross_layers=LC, pos_weight=pw, **KW[name]), max_batch=B_, init="none",
                    adam="lazy", sample_weight=True)
    eng.load_params({k: v.copy() for k, v in P0.items()})
    gz, gl = _run(eng, bs)
    _check(eng, gz, gl, zs, losses, P, "weighted")


# --------------------------------------------------------------------------- 4. predict and persistence
def _trained(name="dnn_pipeline", steps=3, **ekw):
    eng = CTREngine(ModelSpec(name, cross_layers=LC, **KW[name]), max_batch=B_, seed=9, **(ekw or {"adam": "lazy"}))
    bs = _batches(name, steps + 3, seed=40)
    for b in bs[:steps]:
        eng.train_step(b, graph=True)
    torch.cuda.synchronize()
    return eng, bs


def test_predict_on_planes_equals_the_record_path(hip_lib, trajectories):
    """Lazy tables: predict right after training (the batch's records gathered, the first layer
    gathering x0's deep columns itself), after flush() (the flat record lookup) and after
    flush(planes=True) (the plane lookup, unfused because the cross reads x0) give the same bits,
    and they are the restatement's logits within 1e-5."""
    eng, bs = _trained()
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
    cfg = R.make_cfg("dnn_pipeline", **KW["dnn_pipeline"])
    ref = X.forward_backward(cfg, eng.params(), b, LC)
    assert np.abs(z0 - ref["z"]).max() < TOL


def test_checkpoint_and_export_round_trip(hip_lib, tmp_path):
    """A checkpoint saved after three steps and restored into a fresh model continues the
    trajectory bit for bit (logits of two more steps, every parameter, the cross moments); the
    exported model loads with its cross_layers and scores identically."""
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
                                 cross_layers=LC)
    bs = _batches("dnn_pipeline", 5, seed=60)
    a = DeepModel(args, bs)
    a.model_optimizer()
    assert a.engine.cross == LC
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
    for k in X.cross_keys(LC):
        np.testing.assert_array_equal(sa["v"][k], sr["v"][k], err_msg=k)
        np.testing.assert_array_equal(sa["m"][k], sr["m"][k], err_msg=k)
    export_model(a.engine, args.model_pb)
    loaded = load_model(args.model_pb)
    assert loaded.spec.cross_layers == LC and loaded.cross == LC
    np.testing.assert_array_equal(loaded.predict(bs[0]), a.engine.predict(bs[0]))


def test_local_run_train_then_predict(hip_lib, tmp_path):
    """local_run.py dnn_pipeline ... cross_layers=2: train -> export -> predict end to end; the
    exported variables hold the cross vectors and the printed AUC is the restatement's on them
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
            "batch_size=64", "hidden_units=32,16", "shuffle=0", "cross_layers=2"]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "local_run.py")] + args, capture_output=True, text=True,
                       timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "cross_layers = 2" in r.stdout
    auc_gpu = float(r.stdout.split("val of auc:")[-1].split()[0])
    d = np.load(tmp_path / "model_pb" / "variables.npz")
    P = {k: d[k] for k in d.files}
    assert set(X.cross_keys(2)) <= set(P) and P["cross_res"].shape == (13 + 26 * 8, 1)
    kw = dict(C=13, V=0, S=26, E=8, cate_index_size=V, hidden=[32, 16])
    b = {k: v[:192] for k, v in pred_part.items()}
    ref = X.forward_backward(R.make_cfg("dnn_pipeline", **kw), P, b, 2)
    assert abs(R.auc(b["label"], ref["p"]) - auc_gpu) < 1e-4


# --------------------------------------------------------------------------- 5. the default
@pytest.mark.parametrize("adam", ["dense", "lazy"])
def test_default_queues_the_kernels_it_queued(hip_lib, adam, monkeypatch):
    """cross_layers = 0: a step's and a predict's entry-point sequence equals that of an engine
    built without the argument, and holds none of the new entry points or buffers; with
    cross_layers = 2 the same sequence plus the four new launches."""
    from deep_learning_amd import engine as E
    names = []
    real = E.call
    monkeypatch.setattr(E, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    name = "dnn_pipeline"
    bs = _batches(name, 2, seed=70)
    seqs = []
    for extra in ({}, {"cross_layers": 0}, {"cross_layers": LC}):
        eng = CTREngine(ModelSpec(name, **extra, **KW[name]), max_batch=B_, seed=3, adam=adam)
        del names[:]
        eng.train_step(bs[0])
        eng.predict(bs[1])
        torch.cuda.synchronize()
        seqs.append(list(names))
        if not extra.get("cross_layers"):
            assert "cross" not in eng.groups and not any(hasattr(eng, a) for a in ("z_cross", "cross_s"))
    assert seqs[0] == seqs[1] and len(seqs[0]) > 8
    assert not any("cross" in n for n in seqs[0])
    new = ["dl_cross_fwd", "dl_head_fwd_bwd_cross", "dl_cross_bwd", "dl_adam_dense"]
    rest = list(seqs[2])
    for n in new + ["dl_cross_fwd", "dl_head_fwd_bwd_cross"]:      # the step's four, predict's two
        rest.remove(n)
    assert rest == [n for n in seqs[0] if n != "dl_head_fwd_bwd"]
    assert seqs[0].count("dl_head_fwd_bwd") == 2
