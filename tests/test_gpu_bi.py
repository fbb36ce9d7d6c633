"""GPU checks of the Bi-Interaction pooling (ModelSpec.bi_interaction, csrc/bi.hip):
dl_bi_fwd / dl_bi_bwd against the float64 closed forms (tests/_bi_ref.py); five-step trajectories of the
four dnn_* models against the float64 restatement in every table mode, with batch normalisation (the
NFM configuration), with the cross network and the attention, with the product layer, with sample
weights and with later-layer dropout; predict, checkpoint, export and local_run; and the unchanged
kernel sequence at bi_interaction = False.

Kernel shapes (F, E): (2, 4) the smallest of both, one column group a sample; (3, 8) odd F; (26, 16) the
flagship's fields; (33, 8) one field past four unrolled loads of eight (and past eight of the backward's
four); (64, 32) the largest F; (5, 64) the largest E, 16 sample lanes a block; B = 1, 63, 300 (one
sample, a partial block, ten blocks of 32 samples with a partial last one).  The fields start at column
3 of x0 and q follows them, so these runs take the 4-B access form; the engine runs (column 0, pitches of
16 floats) and the aligned case below take the 16-B form."""
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
from tests import _bi_ref as Bi
from tests import _dropout_ref as D
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
SHAPES = [(2, 4), (3, 8), (26, 16), (33, 8), (64, 32), (5, 64)]
EMB_SCALE = 0.3     # injected table: q ~ 0.1 a column, so the pooling moves the logits far beyond the tolerance


def _s():
    return _lib.stream_handle()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


# --------------------------------------------------------------------------- 1. the kernels
def _run_kernels(x, dq, runs=1, x_col0=3, dx_col0=2, tail=5):
    """dl_bi_fwd then dl_bi_bwd on a fixture: x0 [B + 1, x_col0 + (F + 1) E + tail] pre-filled with 7, the
    fields from column x_col0 and q written after them into the same matrix; dx0 [B + 1, dx_col0 + (F + 1) E
    + 3] pre-filled with noise, the fields from dx_col0 and dq after them in the same matrix.  Returns per
    run (x0, dx0) and the pre-filled images."""
    B, F, E = x.shape
    ld = x_col0 + (F + 1) * E + tail
    x0 = np.full((B + 1, ld), 7.0, np.float32)
    x0[:B, x_col0:x_col0 + F * E] = x.reshape(B, F * E)
    dx_ld = dx_col0 + (F + 1) * E + 3
    pre = (np.random.default_rng(5).standard_normal((B + 1, dx_ld)) * 0.1).astype(np.float32)
    pre[:B, dx_col0 + F * E:dx_col0 + (F + 1) * E] = dq
    outs = []
    for _ in range(runs):
        X0 = torch.from_numpy(x0).cuda()
        dx = torch.from_numpy(pre).cuda()
        call("dl_bi_fwd", B, F, E, ptr(X0), ld, x_col0, ptr(X0), ld, x_col0 + F * E, _s())
        call("dl_bi_bwd", B, F, E, ptr(X0), ld, x_col0, ptr(dx), dx_ld, dx_col0 + F * E, ptr(dx), dx_ld, dx_col0, _s())
        torch.cuda.synchronize()
        outs.append((X0.cpu().numpy(), dx.cpu().numpy()))
    return outs, x0, pre


def _check_kernels(x, dq, pad, **geo):
    B, F, E = x.shape
    q64, de64 = Bi.bi_fwd64(x), Bi.bi_bwd64(x, dq)
    if pad is not None:
        assert (q64[pad] == 0).all() and (de64[pad] == 0).all()
    outs, x0, pre = _run_kernels(x, dq, runs=2, **geo)
    for a, b in zip(outs[0], outs[1]):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    xg, dxg = outs[0]
    xc, dc = geo.get("x_col0", 3), geo.get("dx_col0", 2)
    qlo, qhi = xc + F * E, xc + (F + 1) * E
    # the forward wrote q and nothing else (the fields, the pads, the row past B)
    assert np.array_equal(_bits(xg[:, :qlo]), _bits(x0[:, :qlo])) and np.array_equal(_bits(xg[:, qhi:]), _bits(x0[:, qhi:]))
    assert np.array_equal(_bits(xg[B]), _bits(x0[B]))
    # the backward rewrote the field columns and nothing else (the columns before, dq, the columns after, the row past B)
    lo, hi = dc, dc + F * E
    assert np.array_equal(_bits(dxg[:, :lo]), _bits(pre[:, :lo])) and np.array_equal(_bits(dxg[:, hi:]), _bits(pre[:, hi:]))
    assert np.array_equal(_bits(dxg[B]), _bits(pre[B]))
    if pad is not None:
        assert (xg[pad, qlo:qhi] == 0).all()
        assert np.array_equal(_bits(dxg[pad]), _bits(pre[pad]))
    assert np.abs(q64).max() > 0.01 and np.abs(de64).max() > 0
    err = dict(q=np.abs(xg[:B, qlo:qhi] - q64).max(),
               dx0=np.abs(dxg[:B, lo:hi] - (pre[:B, lo:hi].astype(np.float64) + de64.reshape(B, F * E))).max())
    print("(B, F, E) =", (B, F, E), "max |kernel - fp64|:", {k: float(v) for k, v in err.items()})
    for k, v in err.items():
        assert v < TOL, (k, v)


@pytest.mark.parametrize("B", [1, 63, 300])
@pytest.mark.parametrize("F,E", SHAPES)
def test_bi_kernels_match_fp64(hip_lib, F, E, B):
    """q and dx0's addend within 1e-5 (absolute) of the float64 closed forms; the all-padding sample has
    q = 0 and its dx0 row keeps its bits; every column other than q (forward) and the fields (backward)
    keeps its bits, the dq columns and the rows past B included; two runs give the same bits.  Measured
    worst errors: DESIGN 4o."""
    x, dq, pad = Bi.kernel_fixture(B, F, E, seed=1000 * F + E + B)
    _check_kernels(x, dq, pad)


def test_bi_kernels_in_the_aligned_form(hip_lib):
    """The same at the engine's geometry (columns and pitches multiples of 16 B: the 16-B access form),
    and the two forms give q the same bits (dx0's pre-filled noise differs with the geometry)."""
    x, dq, pad = Bi.kernel_fixture(300, 26, 16, seed=77)
    _check_kernels(x, dq, pad, x_col0=0, dx_col0=0, tail=16)
    (a,), _, _ = _run_kernels(x, dq, x_col0=0, dx_col0=0, tail=16)
    (b,), _, _ = _run_kernels(x, dq)
    F, E = 26, 16
    assert np.array_equal(_bits(a[0][:300, F * E:(F + 1) * E]), _bits(b[0][:300, 3 + F * E:3 + (F + 1) * E]))
    assert 1 <= _lib.lib().dl_bi_grid(300) == 10 and _lib.lib().dl_bi_grid(1 << 20) == 1024
    assert _lib.lib().dl_bi_grid(1) == 1 and _lib.lib().dl_bi_grid(65536) == 1024


def test_bi_kernels_refuse_what_they_cannot_take(hip_lib):
    t = torch.full((8, 4400), 3.0, device="cuda")
    o = torch.full((8, 4400), 3.0, device="cuda")
    for F, E in ((1, 8), (65, 8), (4, 6), (4, 0), (4, 68), (4, 2)):
        with pytest.raises(_lib.DLError, match="F %d fields|E %d not" % (F, E)):
            call("dl_bi_fwd", 8, F, E, ptr(t), 4400, 0, ptr(o), 4400, 0, _s())
        with pytest.raises(_lib.DLError, match="F %d fields|E %d not" % (F, E)):
            call("dl_bi_bwd", 8, F, E, ptr(t), 4400, 0, ptr(o), 4400, 4000, ptr(o), 4400, 0, _s())
    with pytest.raises(_lib.DLError, match="field columns"):     # fields past x0's row
        call("dl_bi_fwd", 8, 4, 8, ptr(t), 4400, 4390, ptr(o), 4400, 0, _s())
    with pytest.raises(_lib.DLError, match="within ldq"):        # q past its row
        call("dl_bi_fwd", 8, 4, 8, ptr(t), 4400, 0, ptr(o), 4400, 4396, _s())
    with pytest.raises(_lib.DLError, match="overlap the field columns"):
        call("dl_bi_fwd", 8, 4, 8, ptr(t), 4400, 0, ptr(t), 4400, 28, _s())
    with pytest.raises(_lib.DLError, match="within lddq"):
        call("dl_bi_bwd", 8, 4, 8, ptr(t), 4400, 0, ptr(o), 4400, 4396, ptr(o), 4400, 0, _s())
    with pytest.raises(_lib.DLError, match="within dx_ld"):
        call("dl_bi_bwd", 8, 4, 8, ptr(t), 4400, 0, ptr(o), 4400, 4000, ptr(o), 4400, 4390, _s())
    with pytest.raises(_lib.DLError, match="overlap dx0's field columns"):
        call("dl_bi_bwd", 8, 4, 8, ptr(t), 4400, 0, ptr(o), 4400, 28, ptr(o), 4400, 0, _s())
    torch.cuda.synchronize()
    assert (t == 3).all() and (o == 3).all()


# --------------------------------------------------------------------------- 2. the engine
def _batches(name, n, seed=11, B=B_, kw=None):
    return [Bi.X.make_batch(name, kw or KW[name], B, seed + i) for i in range(n)]


def _init(name, seed, kw=None, **opts):
    """Injected parameters at the models' init scales, the table at EMB_SCALE."""
    cfg = R.make_cfg(name, **(kw or KW[name]))
    rng = np.random.default_rng(seed)
    P = Bi.init_params(cfg, rng, bi=True, theta_scale=0.3, **opts)
    P["feats_emb"] = (rng.standard_normal(P["feats_emb"].shape) * EMB_SCALE).astype(np.float32)
    return cfg, P


def _ref_run(name, P0, bs, kw=None, per_step=None, **opts):
    cfg = R.make_cfg(name, **(kw or KW[name]))
    P = {k: v.copy() for k, v in P0.items()}
    opt = R.AdamTF1(cfg, P)
    zs, losses = [], []
    for i, b in enumerate(bs):
        fw = Bi.train_step(cfg, P, opt, b, bi=True, **opts, **(per_step(i, b) if per_step else {}))
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
    assert got["deep_0"].shape == P["deep_0"].shape == (eng.spec.deep_in, eng.spec.hidden[0])
    err["params"] = max(np.abs(got[k] - P[k]).max() for k in P)
    E = eng.spec.E
    err["deep_0_q_rows"] = np.abs(got["deep_0"][-E:] - P["deep_0"][-E:]).max()
    print(tag, "max |engine - restatement|:", {k: float(v) for k, v in err.items()})
    for k, v in err.items():
        assert v < TOL, (k, v)
    return got


@pytest.mark.parametrize("name", list(KW))
def test_trajectory_matches_restatement(hip_lib, trajectories, name):
    """Five steps (two eager, three replayed as a hipGraph) in every table mode: each step's logits and
    loss and the final parameters (deep_0 with its q rows among them) within 1e-5 of the restatement;
    lazy and sorted + dense bit for bit (dnn_pipeline, dnn_cate: the multi-hot models' dense pooled
    scatter is atomic)."""
    P0, bs, zs, losses, P = trajectories[name]
    res = {}
    for mode, ekw in MODES.items():
        eng = CTREngine(ModelSpec(name, bi_interaction=True, **KW[name]), max_batch=B_, init="none", **ekw)
        assert eng.bi and not eng.fused_gather_rows() and not eng.fused_gather_l0()
        eng.load_params({k: v.copy() for k, v in P0.items()})
        gz, gl = _run(eng, bs)
        res[mode] = (gz, _check(eng, gz, gl, zs, losses, P, "%s %s" % (name, mode)))
    if "multi_ranges" not in KW[name]:
        for a, b in zip(res["lazy"][0], res["sorted"][0]):
            np.testing.assert_array_equal(a, b)
        for k in res["lazy"][1]:
            np.testing.assert_array_equal(res["lazy"][1][k], res["sorted"][1][k], err_msg=k)
    # the pooling does matter: the same steps without it end elsewhere, and its rows of deep_0 train
    E = KW[name]["E"]
    plain = CTREngine(ModelSpec(name, **KW[name]), max_batch=B_, init="none", adam="lazy")
    plain.load_params(dict({k: v.copy() for k, v in P0.items()}, deep_0=P0["deep_0"][:-E].copy()))
    plain.train_step(bs[0])
    torch.cuda.synchronize()
    assert np.abs(plain.z[:B_].cpu().numpy() - zs[0]).max() > 5 * TOL
    assert np.abs(P["deep_0"][-E:] - P0["deep_0"][-E:]).max() > 100 * TOL


def test_wrong_width_parameters_are_refused(hip_lib):
    name = "dnn_cate"
    _, P0 = _init(name, 1)
    E = KW[name]["E"]
    off = CTREngine(ModelSpec(name, **KW[name]), max_batch=B_, init="none")
    with pytest.raises(ValueError, match="deep_0 has .*bi_interaction=False"):
        off.load_params(P0)
    on = CTREngine(ModelSpec(name, bi_interaction=True, **KW[name]), max_batch=B_, init="none")
    with pytest.raises(ValueError, match="deep_0 has .*bi_interaction=True"):
        on.load_params(dict(P0, deep_0=P0["deep_0"][:-E]))


def test_the_nfm_configuration(hip_lib):
    """bi_interaction + batch_norm (the reference's NFM) on dnn_pipeline, lazy and atomic."""
    name = "dnn_pipeline"
    _, P0 = _init(name, 45, bn=True, jitter=0.2)
    bs = _batches(name, 5, seed=13)
    zs, losses, P = _ref_run(name, P0, bs, bn=True)
    for mode in ("atomic", "lazy"):
        eng = CTREngine(ModelSpec(name, bi_interaction=True, batch_norm=True, **KW[name]), max_batch=B_, init="none",
                        **MODES[mode])
        eng.load_params({k: v.copy() for k, v in P0.items()})
        gz, gl = _run(eng, bs)
        _check(eng, gz, gl, zs, losses, P, "nfm %s" % mode)


def test_with_the_cross_network_and_the_attention(hip_lib):
    """dnn_multi with cross_layers = 2 (on the wider input, q included) and afm_attention = 4 as well."""
    name = "dnn_multi"
    _, P0 = _init(name, 43, L=2, A=4)
    assert P0["cross_res"].shape[0] == Bi.deep_in(R.make_cfg(name, **KW[name]), True)
    bs = _batches(name, 5, seed=15)
    zs, losses, P = _ref_run(name, P0, bs, L=2, A=4)
    eng = CTREngine(ModelSpec(name, bi_interaction=True, afm_attention=4, cross_layers=2, **KW[name]), max_batch=B_,
                    init="none", adam="lazy")
    eng.load_params({k: v.copy() for k, v in P0.items()})
    gz, gl = _run(eng, bs)
    _check(eng, gz, gl, zs, losses, P, "cross + afm + bi")


def test_with_the_product_layer(hip_lib):
    name = "dnn_multi_cate"
    _, P0 = _init(name, 46, pnn=True)
    bs = _batches(name, 5, seed=19)
    zs, losses, P = _ref_run(name, P0, bs, pnn=True)
    eng = CTREngine(ModelSpec(name, bi_interaction=True, pnn="inner", **KW[name]), max_batch=B_, init="none",
                    adam="lazy")
    eng.load_params({k: v.copy() for k, v in P0.items()})
    gz, gl = _run(eng, bs)
    _check(eng, gz, gl, zs, losses, P, "pnn + bi")


def test_same_seed_runs_agree_bit_for_bit(hip_lib):
    """Device-initialised engines of one seed, five graph steps each: logits and every parameter equal bit
    for bit; deep_0 is drawn at the new fan-in."""
    name = "dnn_multi"
    bs = _batches(name, 5, seed=3)
    out = []
    for _ in range(2):
        eng = CTREngine(ModelSpec(name, bi_interaction=True, **KW[name]), max_batch=B_, seed=7, adam="lazy")
        p0 = eng.params()
        zs, _ = _run(eng, bs, graph_from=0)
        out.append((zs, eng.params(), p0))
    for a, b in zip(out[0][0], out[1][0]):
        np.testing.assert_array_equal(a, b)
    for k in out[0][1]:
        np.testing.assert_array_equal(out[0][1][k], out[1][1][k], err_msg=k)
    w0 = out[0][2]["deep_0"]
    D0 = 6 * 8 + 5 + 2 + 8
    assert w0.shape == (D0, 32) and 0.7 < w0.std() / np.sqrt(2.0 / (D0 + 32)) < 1.3 and np.abs(w0[-8:]).min() > 0


def test_later_layer_dropout_with_the_pooling(hip_lib):
    """dnn_cate with dropout after the second hidden layer: five lazy steps against the restatement fed
    the masks of the header's words (tests/_dropout_ref.py)."""
    name, seed, keeps = "dnn_cate", 77, [1.0, 1.0, 0.7]
    _, P0 = _init(name, 4)
    bs = _batches(name, 5, seed=21)
    dims = KW[name]["hidden"]

    def per_step(i, b):
        masks = [None, None, D.keep_mask(seed, i + 1, 2, B_, dims[1], keeps[2])]
        return dict(masks=masks, invs=[None, None, D.inv_keep(keeps[2])])
    zs, losses, P = _ref_run(name, P0, bs, per_step=per_step)
    eng = CTREngine(ModelSpec(name, bi_interaction=True, dropout_keep_deep=keeps, **KW[name]), max_batch=B_,
                    init="none", adam="lazy", seed=seed)
    eng.load_params({k: v.copy() for k, v in P0.items()})
    gz, gl = _run(eng, bs)
    _check(eng, gz, gl, zs, losses, P, "dropout")


def test_sample_weights_with_the_pooling(hip_lib):
    """dnn_pipeline with sample_weight=True and pos_weight 2.5 (weights in {0, 0.5, 1, 3}): five lazy
    steps against the restatement's weighted loss."""
    name, pw = "dnn_pipeline", 2.5
    _, P0 = _init(name, 6)
    bs = _batches(name, 5, seed=31)
    for i, b in enumerate(bs):
        b["weight"] = np.random.default_rng(90 + i).choice(np.float32([0, 0.5, 1, 3]), B_).reshape(B_, 1)
    per_step = lambda i, b: dict(w=W.w_eff_f32(b["weight"], b["label"], pw)[0])
    zs, losses, P = _ref_run(name, P0, bs, per_step=per_step)
    eng = CTREngine(ModelSpec(name, bi_interaction=True, pos_weight=pw, **KW[name]), max_batch=B_, init="none",
                    adam="lazy", sample_weight=True)
    eng.load_params({k: v.copy() for k, v in P0.items()})
    gz, gl = _run(eng, bs)
    _check(eng, gz, gl, zs, losses, P, "weighted")


# --------------------------------------------------------------------------- 3. predict and persistence
def test_predict_on_planes_equals_the_record_path(hip_lib):
    """Lazy tables: predict right after training, after flush() and after flush(planes=True) (the plane
    lookup, unfused because the pooling reads x0) give the same bits, and they are the restatement's
    logits within 1e-5."""
    name = "dnn_pipeline"
    eng = CTREngine(ModelSpec(name, bi_interaction=True, **KW[name]), max_batch=B_, init="none", adam="lazy")
    _, P0 = _init(name, 9)
    eng.load_params(P0)
    bs = _batches(name, 6, seed=40)
    for b in bs[:3]:
        eng.train_step(b, graph=True)
    torch.cuda.synchronize()
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
    ref = Bi.forward_backward(R.make_cfg(name, **KW[name]), eng.params(), b, bi=True)
    assert np.abs(z0 - ref["z"]).max() < TOL


def test_checkpoint_and_export_round_trip(hip_lib, tmp_path):
    """A checkpoint saved after three steps and restored into a fresh model continues the trajectory bit
    for bit (logits of two more steps, every parameter); the exported model loads with its bi_interaction
    and scores identically."""
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
                                 bi_interaction=True)
    bs = _batches("dnn_pipeline", 5, seed=60)
    a = DeepModel(args, bs)
    a.model_optimizer()
    assert a.engine.bi is True
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
    export_model(a.engine, args.model_pb)
    loaded = load_model(args.model_pb)
    assert loaded.spec.bi_interaction is True and loaded.bi is True
    np.testing.assert_array_equal(loaded.predict(bs[0]), a.engine.predict(bs[0]))


def test_local_run_train_then_predict(hip_lib, tmp_path):
    """local_run.py dnn_pipeline ... bi_interaction=1 batch_norm=1 (NFM): train -> export -> predict end to
    end; the exported deep_0 has the E more rows and the printed AUC is the restatement's on the exported
    variables within 1e-4."""
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
            "batch_size=64", "hidden_units=32,16", "shuffle=0", "bi_interaction=1", "batch_norm=1"]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "local_run.py")] + args, capture_output=True, text=True,
                       timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    auc_gpu = float(r.stdout.split("val of auc:")[-1].split()[0])
    d = np.load(tmp_path / "model_pb" / "variables.npz")
    P = {k: d[k] for k in d.files}
    assert P["deep_0"].shape == (13 + 26 * 8 + 8, 32)
    kw = dict(C=13, V=0, S=26, E=8, cate_index_size=V, hidden=[32, 16])
    b = {k: v[:192] for k, v in pred_part.items()}
    ref = Bi.forward_backward(R.make_cfg("dnn_pipeline", **kw), P, b, bn=True, bi=True, train=False)
    assert abs(R.auc(b["label"], ref["p"]) - auc_gpu) < 1e-4


# --------------------------------------------------------------------------- 4. the default
@pytest.mark.parametrize("adam", ["dense", "lazy"])
def test_default_queues_the_kernels_it_queued(hip_lib, adam, monkeypatch):
    """bi_interaction = False: a step's and a predict's entry-point sequence equals that of an engine
    built without the argument, holds none of the new entry points, and x0 / dx0 / deep_0 keep their
    widths; with bi_interaction = True the lazy step loses the first layer's fused row gather and both
    gain the two launches (predict one)."""
    from deep_learning_amd import engine as E
    names = []
    real = E.call
    monkeypatch.setattr(E, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    name = "dnn_pipeline"
    bs = _batches(name, 2, seed=70)
    seqs, shapes = [], []
    for extra in ({}, {"bi_interaction": False}, {"bi_interaction": True}):
        eng = CTREngine(ModelSpec(name, **extra, **KW[name]), max_batch=B_, seed=3, adam=adam)
        del names[:]
        eng.train_step(bs[0])
        eng.predict(bs[1])
        torch.cuda.synchronize()
        seqs.append(list(names))
        shapes.append((tuple(eng.x0.shape), tuple(eng.dx0.shape), tuple(eng.W[0].shape), eng.cont_col, eng.dx_cols))
    assert seqs[0] == seqs[1] and len(seqs[0]) > 8 and shapes[0] == shapes[1]
    assert not any("dl_bi_" in n for n in seqs[0])
    assert shapes[2][3] == shapes[0][3] + 8 and shapes[2][4] == shapes[0][4] + 8
    rest = list(seqs[2])
    for n in ["dl_bi_fwd", "dl_bi_bwd", "dl_bi_fwd"]:   # the step's two, predict's one
        rest.remove(n)
    want = ["dl_gemm_s3_nt_bits" if n == "dl_gemm_s3_nt_gather_rows" else n for n in seqs[0]]
    assert rest == want
    assert ("dl_gemm_s3_nt_gather_rows" in seqs[0]) == (adam == "lazy")
