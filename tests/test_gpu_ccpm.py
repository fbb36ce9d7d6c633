"""GPU checks of the CCPM branch (ModelSpec.ccpm_filters, csrc/ccpm.hip): dl_ccpm_fwd /
dl_ccpm_bwd against the float64 restatement (tests/_ccpm_ref.py); five-step trajectories of the four dnn_*
models against the float64 restatement in every table mode, with the cross network and the attention
(the chained logit), with the Bi-Interaction pooling and batch normalisation, with hidden-layer dropout
and with sample weights; predict, checkpoint, export and local_run; and the unchanged kernel sequence at
ccpm_filters = ().

Kernel shapes (F, E, filters): (2, 8, (1,)) the smallest map, every tap but the centre column padding;
(3, 8, (2,)) an odd width, one column dropped; (9, 8, (2, 3, 2)) three layers down to 1 x 1, odd widths
twice; (26, 16, (4, 4)) the flagship's fields, 13 -> 6; (64, 32, (8, 8)) the limits; B = 1, 63, 300 (a
block a sample), and B = 2,100 at (3, 8, (2,)): past the forward's 2,048 blocks and the slab's 512 rows, so
that a block takes several samples in turn.  A gradient jumps where a ReLU sign or a pool decision differs
between float32 and float64, so the samples the restatement calls undecided (margin in _ccpm_ref.py) get
dz = 0 on both sides; the forward is compared on every sample."""
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
from tests import _ccpm_ref as Cc
from tests import _dropout_ref as D
from tests import _sample_weight_ref as W

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL = 1e-5          # the kernels: relative to the largest reference value of the output compared
TOL = 1e-5          # the engine (tests/test_gpu_parity.py): absolute, on logits, loss and parameters
FL = (2, 2)
KW = {"dnn_pipeline": dict(C=13, V=3, S=8, E=8, cate_index_size=1000, hidden=[16, 16]),
      "dnn_cate": dict(V=2, S=8, E=8, cate_index_size=1000, hidden=[16, 16]),
      "dnn_multi": dict(C=5, V=2, S=4, E=8, cate_index_size=1000, hidden=[16, 16],
                        multi_ranges=[[0, 7, "a"], [7, 12, "b"]]),
      "dnn_multi_cate": dict(V=0, S=4, E=8, cate_index_size=1000, hidden=[16, 16],
                             multi_ranges=[[0, 5, "a"], [5, 6, "b"]])}
MODES = {"atomic": dict(bwd="atomic"), "sorted": dict(bwd="sorted"), "lazy": dict(adam="lazy")}
B_ = 64
EMB_SCALE = 0.3     # injected table: z_ccpm ~ 0.1, far beyond the tolerance


def _s():
    return _lib.stream_handle()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _filters(f):
    return (_lib.C.c_int32 * 3)(*f)


# --------------------------------------------------------------------------- 1. the kernels
def _run_kernels(x, P, filters, dz, x_col0=0, dx_col0=0, ld_extra=5, z_add=None, runs=1, pre_scale=1e-3):
    """dl_ccpm_fwd then dl_ccpm_bwd: x0 [B, x_col0 + F E + ld_extra] (pad 7.0, never read), dx0 pre-filled
    (~ N(0, pre_scale^2): the size of the addend, so that the sum's rounding stays below the bound) and
    wider than the field range.  Returns per run (z, dx, slab), the pre-fill and the grid."""
    B, F, E = x.shape
    ld = x_col0 + F * E + ld_extra
    x0 = np.full((B, ld), 7.0, np.float32)
    x0[:, x_col0:x_col0 + F * E] = x.reshape(B, F * E)
    dx_ld = dx_col0 + F * E + 3
    pre = (np.random.default_rng(5).standard_normal((B, dx_ld)) * pre_scale).astype(np.float32)
    n = Cc.n_params(F, E, filters)
    dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in
           dict(x0=x0, prm=Cc.pack(P, F, E, filters), dz=np.asarray(dz, np.float32)).items()}
    za = torch.from_numpy(z_add).cuda() if z_add is not None else None
    grid = _lib.lib().dl_ccpm_grid(B)
    fl = _filters(filters)
    outs = []
    for _ in range(runs):
        z = torch.full((B + 1,), -7.0, device="cuda")
        dx = torch.from_numpy(pre).cuda()
        slab = torch.full((grid + 1, n), -7.0, device="cuda")
        call("dl_ccpm_fwd", B, F, E, len(filters), fl, ptr(dev["x0"]), ld, x_col0, ptr(dev["prm"]), ptr(za), ptr(z), _s())
        call("dl_ccpm_bwd", B, F, E, len(filters), fl, ptr(dev["x0"]), ld, x_col0, ptr(dev["prm"]), ptr(dev["dz"]),
             ptr(dx), dx_ld, dx_col0, ptr(slab), grid, _s())
        torch.cuda.synchronize()
        outs.append(tuple(t.cpu().numpy() for t in (z, dx, slab)))
    return outs, pre, grid


def _reference(x, P, filters, dz):
    z64, _ = Cc.ccpm_fwd(x, P, filters)
    ddx, G = Cc.ccpm_bwd(x, P, filters, dz)
    return z64, ddx, np.concatenate([G[k].reshape(-1) for k in Cc.keys(filters)])


def _errors(x, ref, out, pre, grid, dx_col0, z_add=None):
    """Errors of z, dx0 (pre-fill + addend) and the slab's column sums, each relative to the largest
    reference value (of z, of the addend, of the gradients); the untouched parts keep their bits."""
    B, F, E = x.shape
    z64, ddx, want = ref
    zg, dxg, slg = out
    assert zg[B] == -7 and (slg[grid] == -7).all()
    lo, hi = dx_col0, dx_col0 + F * E
    assert np.array_equal(_bits(dxg[:, :lo]), _bits(pre[:, :lo])) and np.array_equal(_bits(dxg[:, hi:]), _bits(pre[:, hi:]))
    zref = z64 + (0 if z_add is None else z_add.astype(np.float64))
    rel = lambda got, ref: float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-30))
    return dict(z=rel(zg[:B], zref),
                dx0=float(np.abs(dxg[:, lo:hi] - (pre[:, lo:hi].astype(np.float64) + ddx.reshape(B, F * E))).max()
                          / max(np.abs(ddx).max(), 1e-30)),
                slab=rel(slg[:grid].astype(np.float64).sum(0), want))


@pytest.mark.parametrize("B", [1, 63, 300])
@pytest.mark.parametrize("F,E,filters", Cc.SHAPES)
def test_ccpm_kernels_match_fp64(hip_lib, F, E, filters, B):
    """z (every sample), dx0's sum and the slab's column sums (dp, dK_l, db_l) within 1e-5 relative of the
    float64 restatement; undecided samples carry dz = 0 and are at most 10 % of the case (50 % at
    (64, 32, (8, 8))), one decided sample at least; dx0 is pre-filled, added into, and its columns
    outside the fields keep their bits (ld / dx_ld larger than the rows, the fields from column 3 of x0
    and column 2 of dx0 in the odd-F cases); two runs give the same bits; z_add given equals z_add NULL
    plus the addend, bit for bit.  Measured errors (the CCPM_ERR lines): profiles/ccpm/kernel_errors.txt."""
    x, P, dz = Cc.kernel_fixture(B, F, E, filters, seed=1000 * F + 10 * E + B)
    und = Cc.undecided(x, P, filters)
    print("undecided: %d of %d" % (und.sum(), B))
    assert und.mean() <= (0.5 if (F, E) == (64, 32) else 0.1) and (~und).sum() >= 1
    dz = np.where(und, 0.0, dz).astype(np.float32)
    ref = _reference(x, P, filters, dz)
    assert np.abs(ref[1]).max() > 0 and np.abs(ref[2]).max() > 0
    scale = float(np.abs(ref[1]).max())
    xc, dc = (3, 2) if F % 2 else (0, 0)
    outs, pre, grid = _run_kernels(x, P, filters, dz, x_col0=xc, dx_col0=dc, runs=2, pre_scale=scale)
    assert grid == min(B, 512) and _lib.lib().dl_ccpm_grid(1 << 20) == 512
    for a, b in zip(outs[0], outs[1]):
        assert np.array_equal(_bits(a), _bits(b))
    err = _errors(x, ref, outs[0], pre, grid, dc)
    print("CCPM_ERR F=%d E=%d filters=%r B=%d undecided=%d z=%.3g dx0=%.3g slab=%.3g"
          % (F, E, filters, B, und.sum(), err["z"], err["dx0"], err["slab"]))
    for k, v in err.items():
        assert v < REL, (k, v)
    za = np.random.default_rng(B).standard_normal(B).astype(np.float32)
    (with_add,), _, _ = _run_kernels(x, P, filters, dz, x_col0=xc, dx_col0=dc, z_add=za, pre_scale=scale)
    assert np.array_equal(_bits(with_add[0][:B]), _bits(outs[0][0][:B] + za))
    for a, b in zip(with_add[1:], outs[0][1:]):
        assert np.array_equal(_bits(a), _bits(b))


def test_ccpm_kernels_with_several_samples_a_block(hip_lib):
    """B = 2,100 at (3, 8, (2,)): the forward's grid stops at 2,048 blocks and the backward's at the
    slab's 512 rows, so blocks take up to five samples in turn, reusing their LDS maps and summing the
    parameter gradients across them; the same bound."""
    F, E, filters, B = 3, 8, (2,), 2100
    x, P, dz = Cc.kernel_fixture(B, F, E, filters, seed=21)
    und = Cc.undecided(x, P, filters)
    assert und.mean() <= 0.1
    dz = np.where(und, 0.0, dz).astype(np.float32)
    ref = _reference(x, P, filters, dz)
    outs, pre, grid = _run_kernels(x, P, filters, dz, x_col0=3, dx_col0=2, runs=2, pre_scale=float(np.abs(ref[1]).max()))
    assert grid == 512
    for a, b in zip(outs[0], outs[1]):
        assert np.array_equal(_bits(a), _bits(b))
    err = _errors(x, ref, outs[0], pre, grid, 2)
    print("CCPM_ERR F=%d E=%d filters=%r B=%d undecided=%d z=%.3g dx0=%.3g slab=%.3g"
          % (F, E, filters, B, und.sum(), err["z"], err["dx0"], err["slab"]))
    for k, v in err.items():
        assert v < REL, (k, v)


def test_ccpm_kernels_on_ties_and_zeros(hip_lib):
    """The crafted tie case (dyadic values: every u exact in float32, hundreds of windows whose positive
    maximum is attained two to four times) takes the first maximum as the restatement does; a batch of
    all-zero samples with zero biases has z = 0 exactly, adds nothing to dx0 and leaves a zero slab."""
    F, E, filters, B = 9, 8, (2, 3, 2), 63
    x, P, dz = Cc.tie_fixture(B, F, E, filters, seed=5)
    assert Cc.positive_ties(x, P, filters) > 100
    ref = _reference(x, P, filters, dz)
    assert np.abs(ref[1]).max() > 0
    outs, pre, grid = _run_kernels(x, P, filters, dz, x_col0=3, dx_col0=2, pre_scale=float(np.abs(ref[1]).max()))
    err = _errors(x, ref, outs[0], pre, grid, 2)
    print("CCPM_ERR ties F=%d E=%d filters=%r B=%d z=%.3g dx0=%.3g slab=%.3g"
          % (F, E, filters, B, err["z"], err["dx0"], err["slab"]))
    for k, v in err.items():
        assert v < REL, (k, v)
    P0 = {k: (np.zeros_like(v) if k.endswith("bias") else v) for k, v in P.items()}
    outs, pre, grid = _run_kernels(np.zeros_like(x), P0, filters, dz)
    zg, dxg, slg = outs[0]
    assert (zg[:B] == 0).all() and np.array_equal(_bits(dxg), _bits(pre)) and (slg[:grid] == 0).all()


def test_ccpm_kernels_refuse_what_they_cannot_take(hip_lib):
    t = torch.full((8, 2200), 3.0, device="cuda")
    prm = torch.zeros(8192, device="cuda")
    out = torch.full((64,), 3.0, device="cuda")
    slab = torch.full((8192,), 3.0, device="cuda")
    bad = [(1, 8, (2,)), (65, 8, (2,)), (4, 12, (2,)), (4, 8, ()), (4, 8, (2, 2, 2, 2)), (4, 8, (0,)), (4, 8, (9,)),
           (3, 8, (2, 2))]
    for F, E, f in bad:
        L, fl = len(f), _filters(f[:3])
        pat = "F %d fields|E %d not|L %d layers|C \\d filters|layers halve" % (F, E, L)
        with pytest.raises(_lib.DLError, match=pat):
            call("dl_ccpm_fwd", 8, F, E, L, fl, ptr(t), 2200, 0, ptr(prm), None, ptr(out), _s())
        with pytest.raises(_lib.DLError, match=pat):
            call("dl_ccpm_bwd", 8, F, E, L, fl, ptr(t), 2200, 0, ptr(prm), ptr(out), ptr(t), 2200, 0, ptr(slab), 8, _s())
    fl = _filters((2,))
    with pytest.raises(_lib.DLError, match="field columns"):     # fields past x0's row
        call("dl_ccpm_fwd", 8, 4, 8, 1, fl, ptr(t), 2200, 2190, ptr(prm), None, ptr(out), _s())
    with pytest.raises(_lib.DLError, match="dx0 columns"):
        call("dl_ccpm_bwd", 8, 4, 8, 1, fl, ptr(t), 2200, 0, ptr(prm), ptr(out), ptr(t), 2200, 2190, ptr(slab), 8, _s())
    with pytest.raises(_lib.DLError, match="slab needs"):
        call("dl_ccpm_bwd", 8, 4, 8, 1, fl, ptr(t), 2200, 0, ptr(prm), ptr(out), ptr(t), 2200, 0, ptr(slab), 7, _s())
    torch.cuda.synchronize()
    assert (t == 3).all() and (out == 3).all() and (slab == 3).all()


# --------------------------------------------------------------------------- 2. the engine
def _batches(name, n, seed=11, B=B_):
    return [Cc.X.make_batch(name, KW[name], B, seed + i) for i in range(n)]


def _init(name, seed, filters=FL, **opts):
    """Injected parameters at the models' init scales, the table at EMB_SCALE."""
    cfg = R.make_cfg(name, **KW[name])
    rng = np.random.default_rng(seed)
    P = Cc.init_params(cfg, rng, filters, **opts)
    P["feats_emb"] = (rng.standard_normal(P["feats_emb"].shape) * EMB_SCALE).astype(np.float32)
    return cfg, P


def _ref_run(name, P0, bs, filters=FL, per_step=None, **opts):
    """The restatement's steps; no sample of any step may be undecided (the seeds are chosen so), or the
    float32 engine could take another branch of a ReLU or a pool than the float64 restatement."""
    cfg = R.make_cfg(name, **KW[name])
    P = {k: v.copy() for k, v in P0.items()}
    opt = R.AdamTF1(cfg, P)
    zs, losses = [], []
    for i, b in enumerate(bs):
        before = {k: P[k].copy() for k in Cc.keys(filters)}
        fw = Cc.train_step(cfg, P, opt, b, filters, **opts, **(per_step(i, b) if per_step else {}))
        assert not Cc.undecided(fw["fields"], before, filters, exact_ties_ok=True).any(), "step %d: an undecided sample" % i
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


def _check(eng, got_z, got_l, zs, losses, P, tag, filters=FL):
    err = dict(z=max(np.abs(a - b).max() for a, b in zip(got_z, zs)),
               loss=max(abs(a - b) for a, b in zip(got_l, losses)))
    got = eng.params()
    assert set(got) == set(P)
    for k in Cc.keys(filters):
        assert got[k].shape == P[k].shape, k
    err["params"] = max(np.abs(got[k] - P[k]).max() for k in P)
    err["ccpm"] = max(np.abs(got[k] - P[k]).max() for k in Cc.keys(filters))
    print(tag, "max |engine - restatement|:", {k: float(v) for k, v in err.items()})
    for k, v in err.items():
        assert v < TOL, (k, v)
    return got


@pytest.mark.parametrize("name", list(KW))
def test_trajectory_matches_restatement(hip_lib, trajectories, name):
    """Five steps (two eager, three replayed as a hipGraph) in every table mode: each step's logits and
    loss and the final parameters (the CCPM variables among them) within 1e-5 of the restatement; lazy
    and sorted + dense bit for bit (dnn_pipeline, dnn_cate: the multi-hot models' dense pooled scatter is
    atomic); the same steps without the branch end elsewhere."""
    P0, bs, zs, losses, P = trajectories[name]
    res = {}
    for mode, ekw in MODES.items():
        eng = CTREngine(ModelSpec(name, ccpm_filters=FL, **KW[name]), max_batch=B_, init="none", **ekw)
        eng.load_params({k: v.copy() for k, v in P0.items()})
        gz, gl = _run(eng, bs)
        res[mode] = (gz, _check(eng, gz, gl, zs, losses, P, "%s %s" % (name, mode)), eng.dense_state())
    for mv in ("m", "v"):
        for k in Cc.keys(FL):
            assert np.abs(res["lazy"][2][mv][k]).max() > 0
    if "multi_ranges" not in KW[name]:
        for a, b in zip(res["lazy"][0], res["sorted"][0]):
            np.testing.assert_array_equal(a, b)
        for k in res["lazy"][1]:
            np.testing.assert_array_equal(res["lazy"][1][k], res["sorted"][1][k], err_msg=k)
        for mv in ("m", "v"):
            for k in Cc.keys(FL):
                np.testing.assert_array_equal(res["lazy"][2][mv][k], res["sorted"][2][mv][k], err_msg=k)
    plain = CTREngine(ModelSpec(name, **KW[name]), max_batch=B_, init="none", adam="lazy")
    plain.load_params({k: v.copy() for k, v in P0.items() if not k.startswith("ccpm_")})
    plain.train_step(bs[0])
    torch.cuda.synchronize()
    assert np.abs(plain.z[:B_].cpu().numpy() - zs[0]).max() > 100 * TOL
    assert max(np.abs(P[k] - P0[k]).max() for k in Cc.keys(FL)) > 100 * TOL


def test_with_the_cross_network_and_the_attention(hip_lib):
    """dnn_multi with cross_layers = 2 and afm_attention = 4 as well: one logit carries cross, AFM and
    CCPM, in that order; and with cross_layers alone (z_cross straight into dl_ccpm_fwd)."""
    name = "dnn_multi"
    for seed, opts in ((50, dict(L=2, A=4)), (44, dict(L=2))):
        _, P0 = _init(name, seed, **opts)
        bs = _batches(name, 5, seed=15)
        zs, losses, P = _ref_run(name, P0, bs, **opts)
        eng = CTREngine(ModelSpec(name, ccpm_filters=FL, cross_layers=2, afm_attention=opts.get("A", 0), **KW[name]),
                        max_batch=B_, init="none", adam="lazy")
        eng.load_params({k: v.copy() for k, v in P0.items()})
        gz, gl = _run(eng, bs)
        _check(eng, gz, gl, zs, losses, P, "cross + afm + ccpm" if "A" in opts else "cross + ccpm")


def test_with_the_pooling_and_batch_norm(hip_lib):
    """dnn_pipeline with bi_interaction + batch_norm (NFM's tower) beside the branch, lazy and atomic."""
    name = "dnn_pipeline"
    _, P0 = _init(name, 45, bn=True, bi=True, jitter=0.2)
    bs = _batches(name, 5, seed=13)
    zs, losses, P = _ref_run(name, P0, bs, bn=True, bi=True)
    for mode in ("atomic", "lazy"):
        eng = CTREngine(ModelSpec(name, ccpm_filters=FL, bi_interaction=True, batch_norm=True, **KW[name]),
                        max_batch=B_, init="none", **MODES[mode])
        eng.load_params({k: v.copy() for k, v in P0.items()})
        gz, gl = _run(eng, bs)
        _check(eng, gz, gl, zs, losses, P, "bi + bn " + mode)


def test_with_the_product_layer(hip_lib):
    """dnn_multi_cate with pnn='inner' as well, and two layers down to a 2 x 1 map (6 fields -> 3 -> 1)."""
    name, fl = "dnn_multi_cate", (2, 3)
    _, P0 = _init(name, 46, filters=fl, pnn=True, theta_scale=0.3)
    bs = _batches(name, 5, seed=19)
    zs, losses, P = _ref_run(name, P0, bs, filters=fl, pnn=True)
    eng = CTREngine(ModelSpec(name, ccpm_filters=fl, pnn="inner", **KW[name]), max_batch=B_, init="none", adam="lazy")
    eng.load_params({k: v.copy() for k, v in P0.items()})
    gz, gl = _run(eng, bs)
    _check(eng, gz, gl, zs, losses, P, "pnn + ccpm", filters=fl)


def test_same_seed_runs_agree_bit_for_bit(hip_lib):
    """Device-initialised engines of one seed, five graph steps each: logits, every parameter and the CCPM
    moments equal bit for bit; the CCPM variables are drawn as Keras does (glorot_uniform kernels within
    their limit, zero biases) in the reference's shapes."""
    name, fl = "dnn_multi", (4, 2)
    bs = _batches(name, 5, seed=3)
    out = []
    for _ in range(2):
        eng = CTREngine(ModelSpec(name, ccpm_filters=fl, **KW[name]), max_batch=B_, seed=7, adam="lazy")
        p0 = eng.params()
        zs, _ = _run(eng, bs, graph_from=0)
        out.append((zs, eng.params(), eng.dense_state(), p0))
    for a, b in zip(out[0][0], out[1][0]):
        np.testing.assert_array_equal(a, b)
    for k in out[0][1]:
        np.testing.assert_array_equal(out[0][1][k], out[1][1][k], err_msg=k)
    for k in Cc.keys(fl):
        np.testing.assert_array_equal(out[0][2]["v"][k], out[1][2]["v"][k], err_msg=k)
    p0 = out[0][3]
    for k, shp in Cc.shapes(6, 8, fl).items():
        assert p0[k].shape == shp, k
        if k.endswith("bias"):
            assert (p0[k] == 0).all()
        else:
            rf = 9 if len(shp) == 4 else 1
            lim = np.sqrt(6.0 / (rf * (shp[-2] + shp[-1])))
            assert 0.5 * lim < np.abs(p0[k]).max() <= lim * (1 + 1e-6), (k, np.abs(p0[k]).max(), lim)


def test_hidden_dropout_with_the_branch(hip_lib):
    """dnn_cate with dropout after both hidden layers (the tower input kept): five lazy steps against the
    restatement fed the masks of the header's words (tests/_dropout_ref.py)."""
    name, seed, keeps = "dnn_cate", 77, [1.0, 0.8, 0.7]
    _, P0 = _init(name, 4)
    bs = _batches(name, 5, seed=21)
    dims = KW[name]["hidden"]

    def per_step(i, b):
        masks = [None] + [D.keep_mask(seed, i + 1, l + 1, B_, d, keeps[l + 1]) for l, d in enumerate(dims)]
        return dict(masks=masks, invs=[None] + [D.inv_keep(k) for k in keeps[1:]])
    zs, losses, P = _ref_run(name, P0, bs, per_step=per_step)
    eng = CTREngine(ModelSpec(name, ccpm_filters=FL, dropout_keep_deep=keeps, **KW[name]), max_batch=B_, init="none",
                    adam="lazy", seed=seed)
    eng.load_params({k: v.copy() for k, v in P0.items()})
    gz, gl = _run(eng, bs)
    _check(eng, gz, gl, zs, losses, P, "dropout")


def test_sample_weights_with_the_branch(hip_lib):
    """dnn_pipeline with sample_weight=True and pos_weight 2.5 (weights in {0, 0.5, 1, 3}): five lazy
    steps against the restatement's weighted loss."""
    name, pw = "dnn_pipeline", 2.5
    _, P0 = _init(name, 8)
    bs = _batches(name, 5, seed=31)
    for i, b in enumerate(bs):
        b["weight"] = np.random.default_rng(90 + i).choice(np.float32([0, 0.5, 1, 3]), B_).reshape(B_, 1)
    per_step = lambda i, b: dict(w=W.w_eff_f32(b["weight"], b["label"], pw)[0])
    zs, losses, P = _ref_run(name, P0, bs, per_step=per_step)
    eng = CTREngine(ModelSpec(name, ccpm_filters=FL, pos_weight=pw, **KW[name]), max_batch=B_, init="none",
                    adam="lazy", sample_weight=True)
    eng.load_params({k: v.copy() for k, v in P0.items()})
    gz, gl = _run(eng, bs)
    _check(eng, gz, gl, zs, losses, P, "weighted")


def test_wrong_size_parameters_are_refused(hip_lib):
    name = "dnn_cate"
    _, P0 = _init(name, 1)
    eng = CTREngine(ModelSpec(name, ccpm_filters=(2, 3), **KW[name]), max_batch=B_, init="none", adam="lazy")
    with pytest.raises(ValueError, match="ccpm_filters: ccpm_out.kernel holds 8 values, not 12 x 1"):
        eng.load_params({k: v.copy() for k, v in P0.items()})


# --------------------------------------------------------------------------- 3. predict and persistence
def test_predict_on_planes_equals_the_record_path(hip_lib):
    """Lazy tables: predict right after training, after flush() and after flush(planes=True) (the plane
    lookup, unfused because the branch reads x0) give the same bits, and they are the restatement's
    logits within 1e-5."""
    name = "dnn_pipeline"
    eng = CTREngine(ModelSpec(name, ccpm_filters=FL, **KW[name]), max_batch=B_, seed=9, adam="lazy")
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
    ref = Cc.forward_backward(R.make_cfg(name, **KW[name]), eng.params(), b, FL)
    assert np.abs(z0 - ref["z"]).max() < TOL


def test_checkpoint_and_export_round_trip(hip_lib, tmp_path):
    """A checkpoint saved after three steps and restored into a fresh model continues the trajectory bit
    for bit (logits of two more steps, every parameter, the CCPM moments); the exported model loads with
    its ccpm_filters and scores identically."""
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
                                 ccpm_filters=list(FL))
    bs = _batches("dnn_pipeline", 5, seed=60)
    a = DeepModel(args, bs)
    a.model_optimizer()
    assert a.engine.ccpm == FL
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
    for k in Cc.keys(FL):
        np.testing.assert_array_equal(sa["v"][k], sr["v"][k], err_msg=k)
        np.testing.assert_array_equal(sa["m"][k], sr["m"][k], err_msg=k)
    export_model(a.engine, args.model_pb)
    loaded = load_model(args.model_pb)
    assert loaded.spec.ccpm_filters == FL and loaded.ccpm == FL
    np.testing.assert_array_equal(loaded.predict(bs[0]), a.engine.predict(bs[0]))


def test_local_run_train_then_predict(hip_lib, tmp_path):
    """local_run.py dnn_pipeline ... ccpm_filters=2,2: train -> export -> predict end to end; the exported
    variables hold the CCPM variables and the printed AUC is the restatement's on them within 1e-4."""
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
            "batch_size=64", "hidden_units=32,16", "shuffle=0", "ccpm_filters=2,2"]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "local_run.py")] + args, capture_output=True, text=True,
                       timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "ccpm_filters = [2, 2]" in r.stdout
    auc_gpu = float(r.stdout.split("val of auc:")[-1].split()[0])
    d = np.load(tmp_path / "model_pb" / "variables.npz")
    P = {k: d[k] for k in d.files}
    assert set(Cc.keys(FL)) <= set(P)
    assert P["ccpm_conv_1.kernel"].shape == (3, 3, 2, 2) and P["ccpm_out.kernel"].shape == (2 * 6 * 2, 1)
    kw = dict(C=13, V=0, S=26, E=8, cate_index_size=V, hidden=[32, 16])
    b = {k: v[:192] for k, v in pred_part.items()}
    ref = Cc.forward_backward(R.make_cfg("dnn_pipeline", **kw), P, b, FL)
    assert abs(R.auc(b["label"], ref["p"]) - auc_gpu) < 1e-4


# --------------------------------------------------------------------------- 4. the default
@pytest.mark.parametrize("adam", ["dense", "lazy"])
def test_default_queues_the_kernels_it_queued(hip_lib, adam, monkeypatch):
    """ccpm_filters = (): a step's and a predict's entry-point sequence equals that of an engine built
    without the argument, and holds none of the new entry points or buffers; with ccpm_filters = (2, 2)
    the same sequence plus the new launches."""
    from deep_learning_amd import engine as E
    names = []
    real = E.call
    monkeypatch.setattr(E, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    name = "dnn_pipeline"
    bs = _batches(name, 2, seed=70)
    seqs = []
    for extra in ({}, {"ccpm_filters": ()}, {"ccpm_filters": FL}):
        eng = CTREngine(ModelSpec(name, **extra, **KW[name]), max_batch=B_, seed=3, adam=adam)
        del names[:]
        eng.train_step(bs[0])
        eng.predict(bs[1])
        torch.cuda.synchronize()
        seqs.append(list(names))
        if not extra.get("ccpm_filters"):
            assert "ccpm" not in eng.groups and not hasattr(eng, "z_ccpm")
    assert seqs[0] == seqs[1] and len(seqs[0]) > 8
    assert not any("ccpm" in n or "afm" in n or "cross" in n for n in seqs[0])
    new = ["dl_ccpm_fwd", "dl_head_fwd_bwd_cross", "dl_ccpm_bwd", "dl_adam_dense"]
    rest = list(seqs[2])
    for n in new + ["dl_ccpm_fwd", "dl_head_fwd_bwd_cross"]:      # the step's four, predict's two
        rest.remove(n)
    assert rest == [n for n in seqs[0] if n != "dl_head_fwd_bwd"]
    assert seqs[0].count("dl_head_fwd_bwd") == 2
