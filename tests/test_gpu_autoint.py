"""GPU checks of AutoInt's interacting layers (ModelSpec.autoint_layers, csrc/autoint.hip):
dl_autoint_fwd / dl_autoint_bwd against the float64 closed forms (tests/_autoint_ref.py); five-step
trajectories of the four dnn_* models against the float64 restatement in every table mode, with every other
branch (the chained logit), with the Bi-Interaction pooling and batch normalisation, with the product layer,
with hidden-layer dropout and with sample weights; predict, checkpoint, export and local_run; and the
unchanged kernel sequence at autoint_layers = 0.

Kernel shapes (F, E, Hn, D, L): (2, 8, 1, 8, 1) the smallest; (3, 8, 2, 8, 1) odd F, d = 4; (5, 16, 4, 8, 2)
d = 2, D_0 != D; (26, 16, 2, 16, 2) the flagship's fields; (33, 8, 4, 32, 3) past half a wave, D > E;
(64, 32, 4, 32, 3) every limit at once; B = 1, 63, 300, and B = 4,133 at (3, 8, 2, 8, 1): past the forward's
2,048 blocks and the backward's 512 slab rows, so that a block takes several samples in turn.

The ReLU: the fixture keeps only samples whose every |U| (float64) is at least 1e-5 of the fixture's largest,
so a kernel within the bound decides every ReLU as float64 does, and every kept sample is compared.

Bound: REL = 1e-5 of the largest reference value of the compared output (every inner sum has K <= 64); the
float32 CPU evaluation's error on the same fixture is printed beside it.  Measured:
profiles/autoint/kernel_errors.txt."""
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
from tests import _autoint_ref as Ai
from tests import _dropout_ref as D_
from tests import _sample_weight_ref as W

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL = 1e-5          # the kernels: relative to the largest reference value of the output compared
TOL = 1e-5          # the engine (tests/test_gpu_parity.py): absolute, on logits, loss and parameters
AI = (2, 2, 8)      # autoint_layers, autoint_heads, autoint_dim
AIKW = dict(autoint_layers=2, autoint_heads=2, autoint_dim=8)
KW = {"dnn_pipeline": dict(C=13, V=3, S=8, E=8, cate_index_size=1000, hidden=[16, 16]),
      "dnn_cate": dict(V=2, S=8, E=8, cate_index_size=1000, hidden=[16, 16]),
      "dnn_multi": dict(C=5, V=2, S=4, E=8, cate_index_size=1000, hidden=[16, 16],
                        multi_ranges=[[0, 7, "a"], [7, 12, "b"]]),
      "dnn_multi_cate": dict(V=0, S=4, E=8, cate_index_size=1000, hidden=[16, 16],
                             multi_ranges=[[0, 5, "a"], [5, 6, "b"]])}
MODES = {"atomic": dict(bwd="atomic"), "sorted": dict(bwd="sorted"), "lazy": dict(adam="lazy")}
B_ = 64
EMB_SCALE = 0.3     # injected table: z_autoint ~ 0.1, far beyond the tolerance


def _s():
    return _lib.stream_handle()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


# --------------------------------------------------------------------------- 1. the kernels
def _run_kernels(x, P, Hn, D, L, dz, x_col0=0, dx_col0=0, ld_extra=5, z_add=None, runs=1, pre_scale=1e-3):
    """dl_autoint_fwd then dl_autoint_bwd: x0 [B, x_col0 + F E + ld_extra] (pad 7.0, never read), dx0
    pre-filled (~ N(0, pre_scale^2): the size of the addend) and wider than the field range.  Returns per
    run (z, dx, slab), the pre-fill and the grid."""
    B, F, E = x.shape
    ld = x_col0 + F * E + ld_extra
    x0 = np.full((B, ld), 7.0, np.float32)
    x0[:, x_col0:x_col0 + F * E] = x.reshape(B, F * E)
    dx_ld = dx_col0 + F * E + 3
    pre = (np.random.default_rng(5).standard_normal((B, dx_ld)) * pre_scale).astype(np.float32)
    n = Ai.n_params(F, E, L, D)
    dev = {k: torch.from_numpy(np.array(v, np.float32)).cuda() for k, v in
           dict(x0=x0, prm=Ai.pack(P, F, E, L, D), dz=np.asarray(dz, np.float32)).items()}
    za = torch.from_numpy(z_add).cuda() if z_add is not None else None
    grid = _lib.lib().dl_autoint_grid(B)
    outs = []
    for _ in range(runs):
        z = torch.full((B + 1,), -7.0, device="cuda")
        dx = torch.from_numpy(pre).cuda()
        slab = torch.full((grid + 1, n), -7.0, device="cuda")
        call("dl_autoint_fwd", B, F, E, L, Hn, D, ptr(dev["x0"]), ld, x_col0, ptr(dev["prm"]), ptr(za), ptr(z), _s())
        call("dl_autoint_bwd", B, F, E, L, Hn, D, ptr(dev["x0"]), ld, x_col0, ptr(dev["prm"]), ptr(dev["dz"]),
             ptr(dx), dx_ld, dx_col0, ptr(slab), grid, _s())
        torch.cuda.synchronize()
        outs.append(tuple(t.cpu().numpy() for t in (z, dx, slab)))
    return outs, pre, grid


_REFS = {}


def _reference(B, F, E, Hn, D, L, seed, q_scale=1.0):
    """The fixture, its float64 results (z, dx addend, gradient vector) and the float32 CPU evaluation's
    errors; computed once a case and never changed."""
    key = (B, F, E, Hn, D, L, seed, q_scale)
    if key not in _REFS:
        x, P, dz = Ai.kernel_fixture(B, F, E, Hn, D, L, seed, q_scale=q_scale)
        z64, _, _ = Ai.autoint_fwd64(x, P, L, Hn, D)
        ddx, G = Ai.autoint_bwd64(x, P, L, Hn, D, dz)
        ref = (z64, ddx, np.concatenate([G[k].reshape(-1) for k in Ai.keys(L)]))
        got = Ai.autoint_fwd_bwd32(x, P, L, Hn, D, dz)
        e32 = {k: float(np.abs(g - r.reshape(g.shape)).max() / max(np.abs(r).max(), 1e-300))
               for k, g, r in zip(("z", "dx0", "slab"), got, ref)}
        for a in (x, dz) + ref:
            a.setflags(write=False)
        _REFS[key] = (x, P, dz, ref, e32)
    return _REFS[key]


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


def _assert_within(tag, err, e32):
    """Prints the AUTOINT_ERR line with the CPU's float32 errors, then asserts REL."""
    print("AUTOINT_ERR %s z=%.3g dx0=%.3g slab=%.3g cpu_f32: z=%.3g dx0=%.3g slab=%.3g"
          % (tag, err["z"], err["dx0"], err["slab"], e32["z"], e32["dx0"], e32["slab"]))
    for k, v in err.items():
        assert np.isfinite(v) and v < REL, (k, v)


CASES = [s + (B,) for s in Ai.SHAPES for B in (1, 63, 300)]


@pytest.mark.parametrize("F,E,Hn,D,L,B", CASES)
def test_autoint_kernels_match_fp64(hip_lib, F, E, Hn, D, L, B):
    """z (every sample), dx0's sum and the slab's column sums (dw, dWq .. dWr of every layer) against the
    float64 closed forms; dx0 is pre-filled, added into, and its columns outside the fields keep their bits
    (ld / dx_ld larger than the rows, the fields from column 3 of x0 and column 2 of dx0 in the odd-F cases);
    guard rows after z and the slab; two runs give the same bits; z_add given equals z_add NULL plus the
    addend, bit for bit."""
    x, P, dz, ref, e32 = _reference(B, F, E, Hn, D, L, 1000 * F + 10 * E + B)
    assert np.abs(ref[1]).max() > 0 and np.abs(ref[2]).max() > 0
    scale = float(np.abs(ref[1]).max())
    xc, dc = (3, 2) if F % 2 else (0, 0)
    outs, pre, grid = _run_kernels(x, P, Hn, D, L, dz, x_col0=xc, dx_col0=dc, runs=2, pre_scale=scale)
    assert grid == min(B, 512) and _lib.lib().dl_autoint_grid(1 << 20) == 512
    for a, b in zip(outs[0], outs[1]):
        assert np.array_equal(_bits(a), _bits(b))
    _assert_within("F=%d E=%d Hn=%d D=%d L=%d B=%d" % (F, E, Hn, D, L, B), _errors(x, ref, outs[0], pre, grid, dc), e32)
    za = np.random.default_rng(B).standard_normal(B).astype(np.float32)
    (with_add,), _, _ = _run_kernels(x, P, Hn, D, L, dz, x_col0=xc, dx_col0=dc, z_add=za, pre_scale=scale)
    assert np.array_equal(_bits(with_add[0][:B]), _bits(outs[0][0][:B] + za))
    for a, b in zip(with_add[1:], outs[0][1:]):
        assert np.array_equal(_bits(a), _bits(b))


def test_autoint_kernels_with_several_samples_a_block(hip_lib):
    """B = 4,133 at (3, 8, 2, 8, 1): past the forward's 2,048 blocks and the backward's 512 slab rows, so
    blocks take up to nine samples in turn, reusing their LDS and accumulating the weight gradients in
    registers across them; the same bound."""
    F, E, Hn, D, L, B = 3, 8, 2, 8, 1, 4133
    x, P, dz, ref, e32 = _reference(B, F, E, Hn, D, L, 21)
    outs, pre, grid = _run_kernels(x, P, Hn, D, L, dz, x_col0=3, dx_col0=2, runs=2, pre_scale=float(np.abs(ref[1]).max()))
    assert grid == 512
    for a, b in zip(outs[0], outs[1]):
        assert np.array_equal(_bits(a), _bits(b))
    _assert_within("F=%d E=%d Hn=%d D=%d L=%d B=%d" % (F, E, Hn, D, L, B), _errors(x, ref, outs[0], pre, grid, 2), e32)


def test_autoint_kernels_with_large_scores(hip_lib):
    """Wq_1 times 50: scores past 200 (exp would overflow without the row's maximum subtracted); everything
    stays finite and inside the bound."""
    F, E, Hn, D, L, B = 5, 16, 4, 8, 2, 63
    x, P, dz, ref, e32 = _reference(B, F, E, Hn, D, L, 83, q_scale=50.0)     # the first seed from 77 whose scores pass 200
    c = Ai.autoint_fwd64(x, P, L, Hn, D)[2][0]
    assert np.abs(np.einsum("bihc,bkhc->bhik", c["Qh"], c["Kh"])).max() > 200
    outs, pre, grid = _run_kernels(x, P, Hn, D, L, dz, pre_scale=float(np.abs(ref[1]).max()))
    assert all(np.isfinite(a).all() for a in outs[0])
    _assert_within("F=%d E=%d Hn=%d D=%d L=%d B=%d Wq x 50" % (F, E, Hn, D, L, B), _errors(x, ref, outs[0], pre, grid, 0), e32)


def test_autoint_kernels_refuse_what_they_cannot_take(hip_lib):
    t = torch.full((8, 2200), 3.0, device="cuda")
    prm = torch.zeros(16384, device="cuda")
    out = torch.full((64,), 3.0, device="cuda")
    slab = torch.full((8 * 16384,), 3.0, device="cuda")
    #      F, E, L, Hn, D
    bad = [(1, 8, 1, 2, 8), (65, 8, 1, 2, 8), (4, 12, 1, 2, 8), (4, 8, 1, 2, 12), (4, 8, 1, 3, 8), (4, 8, 1, 8, 8),
           (4, 8, 0, 2, 8), (4, 8, 4, 2, 8), (4, 8, 1, 2, 64), (4, 4, 1, 2, 8)]
    pat = "F \\d+ fields|E \\d+ not|L \\d+ layers|heads not one of|D \\d+ not one of|below 2"
    for F, E, L, Hn, D in bad:
        with pytest.raises(_lib.DLError, match=pat):
            call("dl_autoint_fwd", 8, F, E, L, Hn, D, ptr(t), 2200, 0, ptr(prm), None, ptr(out), _s())
        with pytest.raises(_lib.DLError, match=pat):
            call("dl_autoint_bwd", 8, F, E, L, Hn, D, ptr(t), 2200, 0, ptr(prm), ptr(out), ptr(t), 2200, 0, ptr(slab), 8, _s())
    with pytest.raises(_lib.DLError, match="field columns"):     # fields past x0's row
        call("dl_autoint_fwd", 8, 4, 8, 1, 2, 8, ptr(t), 2200, 2190, ptr(prm), None, ptr(out), _s())
    with pytest.raises(_lib.DLError, match="dx0 columns"):
        call("dl_autoint_bwd", 8, 4, 8, 1, 2, 8, ptr(t), 2200, 0, ptr(prm), ptr(out), ptr(t), 2200, 2190, ptr(slab), 8, _s())
    with pytest.raises(_lib.DLError, match="slab needs"):
        call("dl_autoint_bwd", 8, 4, 8, 1, 2, 8, ptr(t), 2200, 0, ptr(prm), ptr(out), ptr(t), 2200, 0, ptr(slab), 1, _s())
    torch.cuda.synchronize()
    assert (t == 3).all() and (out == 3).all() and (slab == 3).all()


# --------------------------------------------------------------------------- 2. the engine
def _batches(name, n, seed=11, B=B_):
    return [Ai.X.make_batch(name, KW[name], B, seed + i) for i in range(n)]


def _init(name, seed, ai=AI, **opts):
    """Injected parameters at the models' init scales, the table at EMB_SCALE."""
    cfg = R.make_cfg(name, **KW[name])
    rng = np.random.default_rng(seed)
    P = Ai.init_params(cfg, rng, ai, **opts)
    P["feats_emb"] = (rng.standard_normal(P["feats_emb"].shape) * EMB_SCALE).astype(np.float32)
    return cfg, P


def _ref_run(name, P0, bs, ai=AI, per_step=None, **opts):
    """The restatement's steps; the smallest |U| it saw must lie above 1e-5 of the largest (the seed is picked
    so that it does), so that the engine decides every ReLU alike."""
    cfg = R.make_cfg(name, **KW[name])
    P = {k: v.copy() for k, v in P0.items()}
    opt = R.AdamTF1(cfg, P)
    zs, losses, lo, hi = [], [], np.inf, 0.0
    for i, b in enumerate(bs):
        fw = Ai.train_step(cfg, P, opt, b, ai, **opts, **(per_step(i, b) if per_step else {}))
        zs.append(fw["z"])
        losses.append(fw["loss"])
        lo, hi = min(lo, fw["u_min"]), max(hi, fw["u_max"])
    return zs, losses, P, lo, hi


def _decided(name, seed0, bs, ai=AI, init_opts={}, per_step=None, **opts):
    """Injected parameters from the first seed from seed0 on at which the restatement alone sees every |U|
    of the five steps above 1e-5 of the largest, so that the engine decides every ReLU alike; with the
    restatement's trajectory."""
    for seed in range(seed0, seed0 + 60):
        _, P0 = _init(name, seed, ai=ai, **init_opts)
        zs, losses, P, lo, hi = _ref_run(name, P0, bs, ai=ai, per_step=per_step, **opts)
        if lo > Ai.MARGIN * hi:
            print("AUTOINT_SEED %s %d: min |U| %.3g, max |U| %.3g" % (name, seed, lo, hi))
            return P0, zs, losses, P
    raise AssertionError("no seed from %d on keeps |U| above the margin" % seed0)


@pytest.fixture(scope="module")
def trajectories():
    """The restatement's five steps from injected parameters, once per model."""
    out = {}
    for name in KW:
        bs = _batches(name, 5)
        P0, zs, losses, P = _decided(name, 42, bs)
        out[name] = (P0, bs, zs, losses, P)
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


def _check(eng, got_z, got_l, zs, losses, P, tag, L=AI[0]):
    err = dict(z=max(np.abs(a - b).max() for a, b in zip(got_z, zs)),
               loss=max(abs(a - b) for a, b in zip(got_l, losses)))
    got = eng.params()
    assert set(got) == set(P)
    for k in Ai.keys(L):
        assert got[k].shape == P[k].shape, k
    err["params"] = max(np.abs(got[k] - P[k]).max() for k in P)
    err["autoint"] = max(np.abs(got[k] - P[k]).max() for k in Ai.keys(L))
    print("AUTOINT_ENGINE", tag, "max |engine - restatement|:", {k: float(v) for k, v in err.items()})
    for k, v in err.items():
        assert v < TOL, (k, v)
    return got


@pytest.mark.parametrize("name", list(KW))
def test_trajectory_matches_restatement(hip_lib, trajectories, name):
    """Five steps (two eager, three replayed as a hipGraph) in every table mode: each step's logits and
    loss and the final parameters (the AutoInt variables among them) within 1e-5 of the restatement; lazy
    and sorted + dense bit for bit (dnn_pipeline, dnn_cate: the multi-hot models' dense pooled scatter is
    atomic); the same steps without the branch end elsewhere."""
    P0, bs, zs, losses, P = trajectories[name]
    res = {}
    for mode, ekw in MODES.items():
        eng = CTREngine(ModelSpec(name, **AIKW, **KW[name]), max_batch=B_, init="none", **ekw)
        eng.load_params({k: v.copy() for k, v in P0.items()})
        gz, gl = _run(eng, bs)
        res[mode] = (gz, _check(eng, gz, gl, zs, losses, P, "%s %s" % (name, mode)), eng.dense_state())
    for mv in ("m", "v"):
        for k in Ai.keys(AI[0]):
            assert np.abs(res["lazy"][2][mv][k]).max() > 0
    if "multi_ranges" not in KW[name]:
        for a, b in zip(res["lazy"][0], res["sorted"][0]):
            np.testing.assert_array_equal(a, b)
        for k in res["lazy"][1]:
            np.testing.assert_array_equal(res["lazy"][1][k], res["sorted"][1][k], err_msg=k)
        for mv in ("m", "v"):
            for k in Ai.keys(AI[0]):
                np.testing.assert_array_equal(res["lazy"][2][mv][k], res["sorted"][2][mv][k], err_msg=k)
    plain = CTREngine(ModelSpec(name, **KW[name]), max_batch=B_, init="none", adam="lazy")
    plain.load_params({k: v.copy() for k, v in P0.items() if not k.startswith("autoint_")})
    plain.train_step(bs[0])
    torch.cuda.synchronize()
    assert np.abs(plain.z[:B_].cpu().numpy() - zs[0]).max() > 100 * TOL
    assert min(np.abs(P[k] - P0[k]).max() for k in Ai.keys(AI[0])) > 100 * TOL


def test_with_the_whole_logit_chain(hip_lib):
    """dnn_multi with cross_layers = 2, afm_attention = 4, ccpm_filters = (2, 2) and cin_layers = (4, 3) as
    well: one logit carries cross, AFM, CCPM, CIN and AutoInt, in that order."""
    from tests import _ccpm_ref as Cc
    name, fl, cl = "dnn_multi", (2, 2), (4, 3)
    opts = dict(L=2, A=4, filters=fl, layers=cl)
    for seed in range(50, 70):      # CCPM's ReLU and pool decisions must be decided in every step (its own rule)
        _, P0 = _init(name, seed, **opts)
        bs = _batches(name, 5, seed=15)
        cfg = R.make_cfg(name, **KW[name])
        P = {k: v.copy() for k, v in P0.items()}
        opt = R.AdamTF1(cfg, P)
        zs, losses, ok, lo, hi = [], [], True, np.inf, 0.0
        for b in bs:
            before = {k: P[k].copy() for k in Cc.keys(fl)}
            fw = Ai.train_step(cfg, P, opt, b, AI, **opts)
            ok = ok and not Cc.undecided(fw["fields"], before, fl, exact_ties_ok=True).any()
            zs.append(fw["z"])
            losses.append(fw["loss"])
            lo, hi = min(lo, fw["u_min"]), max(hi, fw["u_max"])
        if ok and lo > Ai.MARGIN * hi:
            break
    assert ok and lo > Ai.MARGIN * hi
    eng = CTREngine(ModelSpec(name, **AIKW, cin_layers=cl, ccpm_filters=fl, cross_layers=2, afm_attention=4,
                              **KW[name]), max_batch=B_, init="none", adam="lazy")
    eng.load_params({k: v.copy() for k, v in P0.items()})
    gz, gl = _run(eng, bs)
    _check(eng, gz, gl, zs, losses, P, "cross + afm + ccpm + cin + autoint")


def test_with_the_pooling_and_batch_norm(hip_lib):
    """dnn_pipeline with bi_interaction + batch_norm (NFM's tower) beside the branch, lazy and atomic."""
    name = "dnn_pipeline"
    bs = _batches(name, 5, seed=13)
    P0, zs, losses, P = _decided(name, 45, bs, init_opts=dict(bn=True, bi=True, jitter=0.2), bn=True, bi=True)
    for mode in ("atomic", "lazy"):
        eng = CTREngine(ModelSpec(name, **AIKW, bi_interaction=True, batch_norm=True, **KW[name]),
                        max_batch=B_, init="none", **MODES[mode])
        eng.load_params({k: v.copy() for k, v in P0.items()})
        gz, gl = _run(eng, bs)
        _check(eng, gz, gl, zs, losses, P, "bi + bn " + mode)


def test_with_the_product_layer(hip_lib):
    """dnn_multi_cate with pnn='inner' as well, three layers of four heads."""
    name, ai = "dnn_multi_cate", (3, 4, 8)
    bs = _batches(name, 5, seed=19)
    P0, zs, losses, P = _decided(name, 46, bs, ai=ai, init_opts=dict(pnn=True, theta_scale=0.3), pnn=True)
    eng = CTREngine(ModelSpec(name, autoint_layers=3, autoint_heads=4, autoint_dim=8, pnn="inner", **KW[name]),
                    max_batch=B_, init="none", adam="lazy")
    eng.load_params({k: v.copy() for k, v in P0.items()})
    gz, gl = _run(eng, bs)
    _check(eng, gz, gl, zs, losses, P, "pnn + autoint", L=3)


def test_same_seed_runs_agree_bit_for_bit(hip_lib):
    """Device-initialised engines of one seed, five graph steps each: logits, every parameter and the
    AutoInt moments equal bit for bit; the matrices are drawn glorot-uniform within their limit, in the
    variables' shapes."""
    name, ai = "dnn_multi", (2, 4, 16)
    bs = _batches(name, 5, seed=3)
    out = []
    for _ in range(2):
        eng = CTREngine(ModelSpec(name, autoint_layers=2, autoint_heads=4, autoint_dim=16, **KW[name]), max_batch=B_,
                        seed=7, adam="lazy")
        p0 = eng.params()
        zs, _ = _run(eng, bs, graph_from=0)
        out.append((zs, eng.params(), eng.dense_state(), p0))
    for a, b in zip(out[0][0], out[1][0]):
        np.testing.assert_array_equal(a, b)
    for k in out[0][1]:
        np.testing.assert_array_equal(out[0][1][k], out[1][1][k], err_msg=k)
    for k in Ai.keys(2):
        np.testing.assert_array_equal(out[0][2]["v"][k], out[1][2]["v"][k], err_msg=k)
    p0 = out[0][3]
    for k, shp in Ai.shapes(6, 8, 2, 16).items():
        assert p0[k].shape == shp, k
        if k == "autoint_res":
            assert 0 < np.abs(p0[k]).max() < 6 * np.sqrt(2.0 / (6 * 16 + 1))
        else:
            lim = np.sqrt(6.0 / (shp[0] + shp[1]))
            assert 0.5 * lim < np.abs(p0[k]).max() <= lim * (1 + 1e-6), (k, np.abs(p0[k]).max(), lim)


def test_hidden_dropout_with_the_branch(hip_lib):
    """dnn_cate with dropout after both hidden layers (the tower input kept): five lazy steps against the
    restatement fed the masks of the header's words (tests/_dropout_ref.py)."""
    name, seed, keeps = "dnn_cate", 77, [1.0, 0.8, 0.7]
    bs = _batches(name, 5, seed=21)
    dims = KW[name]["hidden"]

    def per_step(i, b):
        masks = [None] + [D_.keep_mask(seed, i + 1, l + 1, B_, d, keeps[l + 1]) for l, d in enumerate(dims)]
        return dict(masks=masks, invs=[None] + [D_.inv_keep(k) for k in keeps[1:]])
    P0, zs, losses, P = _decided(name, 4, bs, per_step=per_step)
    eng = CTREngine(ModelSpec(name, **AIKW, dropout_keep_deep=keeps, **KW[name]), max_batch=B_, init="none",
                    adam="lazy", seed=seed)
    eng.load_params({k: v.copy() for k, v in P0.items()})
    gz, gl = _run(eng, bs)
    _check(eng, gz, gl, zs, losses, P, "dropout")


def test_sample_weights_with_the_branch(hip_lib):
    """dnn_pipeline with sample_weight=True and pos_weight 2.5 (weights in {0, 0.5, 1, 3}): five lazy
    steps against the restatement's weighted loss."""
    name, pw = "dnn_pipeline", 2.5
    bs = _batches(name, 5, seed=31)
    for i, b in enumerate(bs):
        b["weight"] = np.random.default_rng(90 + i).choice(np.float32([0, 0.5, 1, 3]), B_).reshape(B_, 1)
    per_step = lambda i, b: dict(w=W.w_eff_f32(b["weight"], b["label"], pw)[0])
    P0, zs, losses, P = _decided(name, 8, bs, per_step=per_step)
    eng = CTREngine(ModelSpec(name, **AIKW, pos_weight=pw, **KW[name]), max_batch=B_, init="none",
                    adam="lazy", sample_weight=True)
    eng.load_params({k: v.copy() for k, v in P0.items()})
    gz, gl = _run(eng, bs)
    _check(eng, gz, gl, zs, losses, P, "weighted")


def test_wrong_size_parameters_are_refused(hip_lib):
    name = "dnn_cate"
    _, P0 = _init(name, 1)
    eng = CTREngine(ModelSpec(name, autoint_layers=2, autoint_heads=2, autoint_dim=16, **KW[name]), max_batch=B_,
                    init="none", adam="lazy")
    with pytest.raises(ValueError, match="autoint_layers: autoint_res holds 64 values, not 128 x 1"):
        eng.load_params({k: v.copy() for k, v in P0.items()})


# --------------------------------------------------------------------------- 3. predict and persistence
def test_predict_on_planes_equals_the_record_path(hip_lib):
    """Lazy tables: predict right after training, after flush() and after flush(planes=True) (the plane
    lookup, unfused because the branch reads x0) give the same bits, and they are the restatement's
    logits within 1e-5."""
    name = "dnn_pipeline"
    eng = CTREngine(ModelSpec(name, **AIKW, **KW[name]), max_batch=B_, seed=9, adam="lazy")
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
    ref = Ai.forward_backward(R.make_cfg(name, **KW[name]), eng.params(), b, AI)
    assert np.abs(z0 - ref["z"]).max() < TOL


def test_checkpoint_and_export_round_trip(hip_lib, tmp_path):
    """A checkpoint saved after three steps and restored into a fresh model continues the trajectory bit
    for bit (logits of two more steps, every parameter, the AutoInt moments); the exported model loads with
    its autoint options and scores identically."""
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
                                 **AIKW)
    bs = _batches("dnn_pipeline", 5, seed=60)
    a = DeepModel(args, bs)
    a.model_optimizer()
    assert a.engine.autoint == 2
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
    for k in Ai.keys(2):
        np.testing.assert_array_equal(sa["v"][k], sr["v"][k], err_msg=k)
        np.testing.assert_array_equal(sa["m"][k], sr["m"][k], err_msg=k)
    export_model(a.engine, args.model_pb)
    loaded = load_model(args.model_pb)
    sp = loaded.spec
    assert (sp.autoint_layers, sp.autoint_heads, sp.autoint_dim) == AI and loaded.autoint == 2
    np.testing.assert_array_equal(loaded.predict(bs[0]), a.engine.predict(bs[0]))


def test_local_run_train_then_predict(hip_lib, tmp_path):
    """local_run.py dnn_pipeline ... autoint_layers=2 autoint_heads=2 autoint_dim=8: train -> export -> predict
    end to end; the exported variables hold the AutoInt variables and the printed AUC is the restatement's
    on them within 1e-4."""
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
            "batch_size=64", "hidden_units=32,16", "shuffle=0", "autoint_layers=2", "autoint_heads=2", "autoint_dim=8"]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "local_run.py")] + args, capture_output=True, text=True,
                       timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "autoint_layers = 2" in r.stdout
    auc_gpu = float(r.stdout.split("val of auc:")[-1].split()[0])
    d = np.load(tmp_path / "model_pb" / "variables.npz")
    P = {k: d[k] for k in d.files}
    assert set(Ai.keys(2)) <= set(P)
    assert P["autoint_q_0"].shape == (8, 8) and P["autoint_r_1"].shape == (8, 8) and P["autoint_res"].shape == (26 * 8, 1)
    kw = dict(C=13, V=0, S=26, E=8, cate_index_size=V, hidden=[32, 16])
    b = {k: v[:192] for k, v in pred_part.items()}
    ref = Ai.forward_backward(R.make_cfg("dnn_pipeline", **kw), P, b, AI)
    assert abs(R.auc(b["label"], ref["p"]) - auc_gpu) < 1e-4


# --------------------------------------------------------------------------- 4. the default
@pytest.mark.parametrize("adam", ["dense", "lazy"])
def test_default_queues_the_kernels_it_queued(hip_lib, adam, monkeypatch):
    """autoint_layers = 0: a step's and a predict's entry-point sequence equals that of an engine built
    without the argument, and holds none of the new entry points or buffers; with the branch on the same
    sequence plus the new launches."""
    from deep_learning_amd import engine as E
    names = []
    real = E.call
    monkeypatch.setattr(E, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    name = "dnn_pipeline"
    bs = _batches(name, 2, seed=70)
    seqs = []
    for extra in ({}, dict(autoint_layers=0, autoint_heads=4, autoint_dim=32), AIKW):
        eng = CTREngine(ModelSpec(name, **extra, **KW[name]), max_batch=B_, seed=3, adam=adam)
        del names[:]
        eng.train_step(bs[0])
        eng.predict(bs[1])
        torch.cuda.synchronize()
        seqs.append(list(names))
        if not extra.get("autoint_layers"):
            assert "autoint" not in eng.groups and not hasattr(eng, "z_autoint") and not eng.autoint
    assert seqs[0] == seqs[1] and len(seqs[0]) > 8
    assert not any("autoint" in n or "cin" in n or "ccpm" in n or "afm" in n or "cross" in n for n in seqs[0])
    new = ["dl_autoint_fwd", "dl_head_fwd_bwd_cross", "dl_autoint_bwd", "dl_adam_dense"]
    rest = list(seqs[2])
    for n in new + ["dl_autoint_fwd", "dl_head_fwd_bwd_cross"]:      # the step's four, predict's two
        rest.remove(n)
    assert rest == [n for n in seqs[0] if n != "dl_head_fwd_bwd"]
    assert seqs[0].count("dl_head_fwd_bwd") == 2
