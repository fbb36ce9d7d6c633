"""GPU checks of the inner-product layer (ModelSpec.pnn, csrc/pnn.hip):
dl_pnn_inner_fwd / dl_pnn_inner_bwd against the float64 formulas (tests/_pnn_ref.py), and the engine
with one hidden layer.  The other engine-level checks (trajectories, predict, checkpoint, export,
local_run, the unchanged kernel sequence at pnn = None) are shared with the
other options: their bodies run on the "pnn" row of tests/_side_options.py, called from the last section
here or collected as the [pnn] cases of tests/test_gpu_side_options.py.

Kernel shapes (F, E, D1): (2, 8, 1) the smallest, two samples a tile; (3, 16, 33) odd F, a partial
third column tile; (26, 16, 50) and (26, 16, 400) the flagship's fields, fewer and more column tiles
than backward waves; (33, 8, 416) three field tiles, theta split into two D1-chunks in the backward;
(64, 32, 48) the largest F and E, two tiles a sample, four backward waves; B = 1, 63, 300 (a
partial last unit, more than one pass of the backward's capped grid)."""
import numpy as np
import pytest
import torch

from deep_learning_amd import _lib
from deep_learning_amd._lib import call, ptr
from tests import _pnn_ref as Pn
from tests._side_options import (MODES, PNN, TOL, _batches, _bits, _check, _engine, _init, _ref_run, _run, _s,
                                  default_queues_the_kernels_it_queued, follow, trajectory_matches_restatement,
                                  with_the)

pytestmark = pytest.mark.gpu

SHAPES = [(2, 8, 1), (3, 16, 33), (26, 16, 50), (26, 16, 400), (33, 8, 416), (64, 32, 48)]
X_COL0, DX_COL0 = 3, 2


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


# --------------------------------------------------------------------------- 2. the engine, what only pnn has
def test_one_hidden_layer_has_no_sign_bitmask(hip_lib):
    """hidden = [24]: the head masks dh[0] by h[0] > 0 itself; dense and lazy."""
    name = "dnn_pipeline"
    kw = dict(PNN.KW[name], hidden=[24])
    _, P0 = _init(PNN, name, 44, kw=kw)
    bs = _batches(PNN, name, 5, seed=17, kw=kw)
    zs, losses, P = _ref_run(PNN, name, P0, bs, kw=kw)
    for mode in ("atomic", "lazy"):
        eng = _engine(PNN, name, kw=kw, init="none", **MODES[mode])
        assert len(eng.hbits) == 0
        eng.load_params({k: v.copy() for k, v in P0.items()})
        gz, gl = _run(eng, bs)
        _check(PNN, eng, gz, gl, zs, losses, P, "one layer %s" % mode)


# --------------------------------------------------------------------------- the engine: the shared bodies
# (tests/_side_options.py) on this option's row
@pytest.mark.parametrize("name", list(PNN.KW))
def test_trajectory_matches_restatement(hip_lib, name):
    trajectory_matches_restatement(PNN, name)


def test_with_the_cross_network_and_the_attention(hip_lib):
    with_the(PNN, "the_cross_network_and_the_attention")


def test_later_layer_dropout_with_the_layer(hip_lib):
    follow(PNN, PNN.dropout)


def test_sample_weights_with_the_layer(hip_lib):
    follow(PNN, PNN.weighted)


@pytest.mark.parametrize("adam", ["dense", "lazy"])
def test_default_queues_the_kernels_it_queued(hip_lib, adam, monkeypatch):
    default_queues_the_kernels_it_queued(PNN, "dnn_pipeline", adam, monkeypatch)
