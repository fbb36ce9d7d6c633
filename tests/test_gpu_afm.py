"""GPU checks of the attentional pairwise interactions (ModelSpec.afm_attention, csrc/afm.hip,
DESIGN 4l): dl_afm_fwd / dl_afm_bwd against the float64 formulas (tests/_afm_ref.py) on the dyadic
fixture.  The engine-level checks (trajectories, predict, checkpoint, export, local_run, the unchanged
kernel sequence at afm_attention = 0) are shared with the
other options: their bodies run on the "afm" row of tests/_side_options.py, called from the last section
here or collected as the [afm] cases of tests/test_gpu_side_options.py.

Kernel shapes (F, E, A): (2, 8, 1) the smallest; (3, 16, 5) odd F, unaligned A; (26, 16, 16) and
(32, 16, 16) two samples a wave, odd and even round counts; (33, 8, 32) one sample a wave, the
largest A; (64, 32, 7) the largest F and E, 2,016 pairs; B = 1, 63, 300 (a partial last group, more
than one pass of the backward's capped grid)."""
import numpy as np
import pytest
import torch

from deep_learning_amd import _lib
from deep_learning_amd._lib import call, ptr
from tests import _afm_ref as Af
from tests._side_options import (AFM, TOL, _bits, _s, default_queues_the_kernels_it_queued, follow,
                                  trajectory_matches_restatement, with_the)

pytestmark = pytest.mark.gpu

SHAPES = [(2, 8, 1), (3, 16, 5), (26, 16, 16), (32, 16, 16), (33, 8, 32), (64, 32, 7)]


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


# --------------------------------------------------------------------------- the engine: the shared bodies
# (tests/_side_options.py) on this option's row
@pytest.mark.parametrize("name", list(AFM.KW))
def test_trajectory_matches_restatement(hip_lib, name):
    trajectory_matches_restatement(AFM, name)


def test_with_the_cross_network(hip_lib):
    with_the(AFM, "the_cross_network")


def test_hidden_dropout_with_the_branch(hip_lib):
    follow(AFM, AFM.dropout)


def test_sample_weights_with_the_branch(hip_lib):
    follow(AFM, AFM.weighted)


@pytest.mark.parametrize("adam", ["dense", "lazy"])
def test_default_queues_the_kernels_it_queued(hip_lib, adam, monkeypatch):
    default_queues_the_kernels_it_queued(AFM, "dnn_pipeline", adam, monkeypatch)
