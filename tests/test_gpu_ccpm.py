"""GPU checks of the CCPM branch (ModelSpec.ccpm_filters, csrc/ccpm.hip): dl_ccpm_fwd /
dl_ccpm_bwd against the float64 restatement (tests/_ccpm_ref.py).  The engine-level checks (trajectories,
predict, checkpoint, export, local_run, the unchanged kernel sequence at ccpm_filters = ())
are shared with the other options: their bodies run on the "ccpm" row of tests/_side_options.py, called from the last section
here or collected as the [ccpm] cases of tests/test_gpu_side_options.py.

Kernel shapes (F, E, filters): (2, 8, (1,)) the smallest map, every tap but the centre column padding;
(3, 8, (2,)) an odd width, one column dropped; (9, 8, (2, 3, 2)) three layers down to 1 x 1, odd widths
twice; (26, 16, (4, 4)) the flagship's fields, 13 -> 6; (64, 32, (8, 8)) the limits; B = 1, 63, 300 (a
block a sample), and B = 2,100 at (3, 8, (2,)): past the forward's 2,048 blocks and the slab's 512 rows, so
that a block takes several samples in turn.  A gradient jumps where a ReLU sign or a pool decision differs
between float32 and float64, so the samples the restatement calls undecided (margin in _ccpm_ref.py) get
dz = 0 on both sides; the forward is compared on every sample."""
import numpy as np
import pytest
import torch

from deep_learning_amd import _lib
from deep_learning_amd._lib import call, ptr
from tests import _ccpm_ref as Cc
from tests._side_options import (CCPM, _bits, _s, default_queues_the_kernels_it_queued, follow,
                                  trajectory_matches_restatement, with_the, wrong_size_parameters_are_refused)

pytestmark = pytest.mark.gpu

REL = 1e-5          # the kernels: relative to the largest reference value of the output compared


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


# --------------------------------------------------------------------------- the engine: the shared bodies
# (tests/_side_options.py) on this option's row
@pytest.mark.parametrize("name", list(CCPM.KW))
def test_trajectory_matches_restatement(hip_lib, name):
    trajectory_matches_restatement(CCPM, name)


def test_with_the_cross_network_and_the_attention(hip_lib):
    with_the(CCPM, "the_cross_network_and_the_attention")


def test_with_the_pooling_and_batch_norm(hip_lib):
    with_the(CCPM, "the_pooling_and_batch_norm")


def test_with_the_product_layer(hip_lib):
    with_the(CCPM, "the_product_layer")


def test_hidden_dropout_with_the_branch(hip_lib):
    follow(CCPM, CCPM.dropout)


def test_sample_weights_with_the_branch(hip_lib):
    follow(CCPM, CCPM.weighted)


def test_wrong_size_parameters_are_refused(hip_lib):
    wrong_size_parameters_are_refused(CCPM)


@pytest.mark.parametrize("adam", ["dense", "lazy"])
def test_default_queues_the_kernels_it_queued(hip_lib, adam, monkeypatch):
    default_queues_the_kernels_it_queued(CCPM, "dnn_pipeline", adam, monkeypatch)
