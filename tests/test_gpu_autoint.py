"""GPU checks of AutoInt's interacting layers (ModelSpec.autoint_layers, csrc/autoint.hip):
dl_autoint_fwd / dl_autoint_bwd against the float64 closed forms (tests/_autoint_ref.py).  The engine-level
checks (trajectories, predict, checkpoint, export, local_run, the unchanged kernel sequence at
autoint_layers = 0) are shared with the
other options: their bodies run on the "autoint" row of tests/_side_options.py, called from the last section
here or collected as the [autoint] cases of tests/test_gpu_side_options.py.

Kernel shapes (F, E, Hn, D, L): (2, 8, 1, 8, 1) the smallest; (3, 8, 2, 8, 1) odd F, d = 4; (5, 16, 4, 8, 2)
d = 2, D_0 != D; (26, 16, 2, 16, 2) the flagship's fields; (33, 8, 4, 32, 3) past half a wave, D > E;
(64, 32, 4, 32, 3) every limit at once; B = 1, 63, 300, and B = 4,133 at (3, 8, 2, 8, 1): past the forward's
2,048 blocks and the backward's 512 slab rows, so that a block takes several samples in turn.

The ReLU: the fixture keeps only samples whose every |U| (float64) is at least 1e-5 of the fixture's largest,
so a kernel within the bound decides every ReLU as float64 does, and every kept sample is compared.

Bound: REL = 1e-5 of the largest reference value of the compared output (every inner sum has K <= 64); the
float32 CPU evaluation's error on the same fixture is printed beside it.  Measured:
profiles/autoint/kernel_errors.txt."""
import numpy as np
import pytest
import torch

from deep_learning_amd import _lib
from deep_learning_amd._lib import call, ptr
from tests import _autoint_ref as Ai
from tests._side_options import (AUTOINT, _bits, _s, default_queues_the_kernels_it_queued, follow,
                                  trajectory_matches_restatement, with_the, wrong_size_parameters_are_refused)

pytestmark = pytest.mark.gpu

REL = 1e-5          # the kernels: relative to the largest reference value of the output compared


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


# --------------------------------------------------------------------------- the engine: the shared bodies
# (tests/_side_options.py) on this option's row
@pytest.mark.parametrize("name", list(AUTOINT.KW))
def test_trajectory_matches_restatement(hip_lib, name):
    trajectory_matches_restatement(AUTOINT, name)


def test_with_the_whole_logit_chain(hip_lib):
    with_the(AUTOINT, "the_whole_logit_chain")


def test_with_the_pooling_and_batch_norm(hip_lib):
    with_the(AUTOINT, "the_pooling_and_batch_norm")


def test_with_the_product_layer(hip_lib):
    with_the(AUTOINT, "the_product_layer")


def test_hidden_dropout_with_the_branch(hip_lib):
    follow(AUTOINT, AUTOINT.dropout)


def test_sample_weights_with_the_branch(hip_lib):
    follow(AUTOINT, AUTOINT.weighted)


def test_wrong_size_parameters_are_refused(hip_lib):
    wrong_size_parameters_are_refused(AUTOINT)


@pytest.mark.parametrize("adam", ["dense", "lazy"])
def test_default_queues_the_kernels_it_queued(hip_lib, adam, monkeypatch):
    default_queues_the_kernels_it_queued(AUTOINT, "dnn_pipeline", adam, monkeypatch)
