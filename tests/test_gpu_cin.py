"""GPU checks of the Compressed Interaction Network (ModelSpec.cin_layers, csrc/cin.hip):
dl_cin_fwd / dl_cin_bwd against the float64 closed forms (tests/_cin_ref.py).  The engine-level checks
(trajectories, predict, checkpoint, export, local_run, the unchanged kernel sequence at cin_layers = ())
are shared with the other options: their bodies run on the "cin" row of tests/_side_options.py, called from the last section
here or collected as the [cin] cases of tests/test_gpu_side_options.py.

Kernel shapes (F, E, layers): (2, 8, (1,)) the smallest; (3, 8, (2,)) odd F, K = 9 no multiple of 4;
(5, 16, (3, 5)) two layers, neither H a multiple of 16, K = 25 and 15; (26, 16, (16, 16)) the flagship's
fields; (16, 8, (64, 64, 64)) three layers at the largest H; (64, 32, (64,)) K = 4,096, a sample a unit
(B = 1 and 63 only: the float64 einsum at 300 is too large for a seconds-long test); B = 1, 63, 300, and
B = 4,133 at (3, 8, (2,)): past the forward's 1,024 blocks of 4 samples and the slab's 128 rows, so that a
block takes several units in turn.

Bound: every layer K <= 1,024: REL = 1e-5 of the largest reference value.  The two large shapes: the same
formulas evaluated in float32 on the CPU (torch einsum) against float64 on the same fixture give e32, and the
GPU's error must stay within max(1e-5, 8 e32) where a layer has K > 1,024 (the last shape; the three-layer
one has K = 1,024 and keeps REL, its e32 printed beside it): a single fma chain rounds about sqrt(vector width) worse than
the CPU's blocked sums.  Measured: profiles/cin/kernel_errors.txt."""
import numpy as np
import pytest
import torch

from deep_learning_amd import _lib
from deep_learning_amd._lib import call, ptr
from tests import _cin_ref as Ci
from tests._side_options import (CIN, _bits, _s, default_queues_the_kernels_it_queued, follow,
                                  trajectory_matches_restatement, with_the, wrong_size_parameters_are_refused)

pytestmark = pytest.mark.gpu

REL = 1e-5          # the kernels: relative to the largest reference value of the output compared


def _layers(h):
    return (_lib.C.c_int32 * 3)(*h)


# --------------------------------------------------------------------------- 1. the kernels
def _run_kernels(x, P, layers, dz, x_col0=0, dx_col0=0, ld_extra=5, z_add=None, runs=1, pre_scale=1e-3):
    """dl_cin_fwd then dl_cin_bwd: x0 [B, x_col0 + F E + ld_extra] (pad 7.0, never read), dx0 pre-filled
    (~ N(0, pre_scale^2): the size of the addend, so that the sum's rounding stays below the bound) and
    wider than the field range.  Returns per run (z, dx, slab), the pre-fill and the grid."""
    B, F, E = x.shape
    ld = x_col0 + F * E + ld_extra
    x0 = np.full((B, ld), 7.0, np.float32)
    x0[:, x_col0:x_col0 + F * E] = x.reshape(B, F * E)
    dx_ld = dx_col0 + F * E + 3
    pre = (np.random.default_rng(5).standard_normal((B, dx_ld)) * pre_scale).astype(np.float32)
    n = Ci.n_params(F, layers)
    dev = {k: torch.from_numpy(np.array(v, np.float32)).cuda() for k, v in
           dict(x0=x0, prm=Ci.pack(P, F, layers), dz=np.asarray(dz, np.float32)).items()}
    za = torch.from_numpy(z_add).cuda() if z_add is not None else None
    grid = _lib.lib().dl_cin_grid(B)
    hl = _layers(layers)
    outs = []
    for _ in range(runs):
        z = torch.full((B + 1,), -7.0, device="cuda")
        dx = torch.from_numpy(pre).cuda()
        slab = torch.full((grid + 1, n), -7.0, device="cuda")
        call("dl_cin_fwd", B, F, E, len(layers), hl, ptr(dev["x0"]), ld, x_col0, ptr(dev["prm"]), ptr(za), ptr(z), _s())
        call("dl_cin_bwd", B, F, E, len(layers), hl, ptr(dev["x0"]), ld, x_col0, ptr(dev["prm"]), ptr(dev["dz"]),
             ptr(dx), dx_ld, dx_col0, ptr(slab), grid, _s())
        torch.cuda.synchronize()
        outs.append(tuple(t.cpu().numpy() for t in (z, dx, slab)))
    return outs, pre, grid


_REFS = {}


def _large(F, layers):
    """The two large shapes, whose float32 evaluation on the CPU is measured beside the GPU's."""
    return max(layers) * F >= 1024


def _max_k(F, layers):
    H = (F,) + tuple(layers)
    return max(H[k] * F for k in range(len(layers)))


def _reference(B, F, E, layers, seed):
    """The fixture, its float64 results (z, dx addend, gradient vector) and, for the large shapes, the
    float32 evaluation's errors; computed once a case and never changed."""
    key = (B, F, E, layers, seed)
    if key not in _REFS:
        x, P, dz = Ci.kernel_fixture(B, F, E, layers, seed)
        z64, _ = Ci.cin_fwd64(x, P, layers)
        ddx, G = Ci.cin_bwd64(x, P, layers, dz)
        ref = (z64, ddx, np.concatenate([G[k].reshape(-1) for k in Ci.keys(layers)]))
        e32 = None
        if _large(F, layers):
            got = Ci.cin_fwd_bwd32(x, P, layers, dz)
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


def _assert_within(tag, err, e32, max_k):
    """Prints the CIN_ERR line (with the CPU's float32 errors where measured), then asserts REL where every
    layer has K <= 1,024, else max(REL, 8 e32)."""
    print("CIN_ERR %s z=%.3g dx0=%.3g slab=%.3g%s"
          % (tag, err["z"], err["dx0"], err["slab"],
             "" if e32 is None else " cpu_f32: z=%.3g dx0=%.3g slab=%.3g" % (e32["z"], e32["dx0"], e32["slab"])))
    for k, v in err.items():
        if max_k <= 1024:
            assert v < REL, (k, v)
        else:
            assert v <= max(REL, 8 * e32[k]), (k, v, e32[k])


CASES = [(F, E, layers, B) for F, E, layers in Ci.SHAPES for B in (1, 63, 300) if not (F == 64 and B == 300)]


@pytest.mark.parametrize("F,E,layers,B", CASES)
def test_cin_kernels_match_fp64(hip_lib, F, E, layers, B):
    """z (every sample), dx0's sum and the slab's column sums (dc, dW^k) against the float64 closed forms;
    dx0 is pre-filled, added into, and its columns outside the fields keep their bits (ld / dx_ld larger
    than the rows, the fields from column 3 of x0 and column 2 of dx0 in the odd-F cases); guard rows after
    z and the slab; two runs give the same bits; z_add given equals z_add NULL plus the addend, bit for
    bit; the all-zero sample's z is exactly 0."""
    x, P, dz, ref, e32 = _reference(B, F, E, layers, 1000 * F + 10 * E + B)
    assert (e32 is not None) == ((F, E) in ((16, 8), (64, 32))) and (_max_k(F, layers) > 1024) == (F == 64)
    assert B == 1 or (np.abs(ref[1]).max() > 0 and np.abs(ref[2]).max() > 0)
    scale = float(np.abs(ref[1]).max()) or 1e-3
    xc, dc = (3, 2) if F % 2 else (0, 0)
    outs, pre, grid = _run_kernels(x, P, layers, dz, x_col0=xc, dx_col0=dc, runs=2, pre_scale=scale)
    assert grid == min((B + 3) // 4, 128) and _lib.lib().dl_cin_grid(1 << 20) == 128
    for a, b in zip(outs[0], outs[1]):
        assert np.array_equal(_bits(a), _bits(b))
    err = _errors(x, ref, outs[0], pre, grid, dc)
    if B == 1:      # the one sample is the all-zero one: nothing to be relative to
        assert outs[0][0][0] == 0 and (outs[0][2][:grid] == 0).all()
        assert np.array_equal(_bits(outs[0][1]), _bits(pre))
        print("CIN_ERR F=%d E=%d layers=%r B=1 all zero: exact" % (F, E, layers))
    else:
        _assert_within("F=%d E=%d layers=%r B=%d" % (F, E, layers, B), err, e32, _max_k(F, layers))
        assert outs[0][0][B // 2] == 0
    za = np.random.default_rng(B).standard_normal(B).astype(np.float32)
    (with_add,), _, _ = _run_kernels(x, P, layers, dz, x_col0=xc, dx_col0=dc, z_add=za, pre_scale=scale)
    assert np.array_equal(_bits(with_add[0][:B]), _bits(outs[0][0][:B] + za))
    for a, b in zip(with_add[1:], outs[0][1:]):
        assert np.array_equal(_bits(a), _bits(b))


@pytest.mark.parametrize("F,E,layers", Ci.SHAPES)
def test_cin_kernels_on_one_live_sample(hip_lib, F, E, layers):
    """B = 1 with a live sample (the fixture's B = 1 is its padding sample): sample 0 of the B = 63 case."""
    x, P, dz, _, _ = _reference(63, F, E, layers, 1000 * F + 10 * E + 63)
    x, dz = x[:1], dz[:1]
    z64, _ = Ci.cin_fwd64(x, P, layers)
    ddx, G = Ci.cin_bwd64(x, P, layers, dz)
    ref = (z64, ddx, np.concatenate([G[k].reshape(-1) for k in Ci.keys(layers)]))
    e32 = None
    if _large(F, layers):
        got = Ci.cin_fwd_bwd32(x, P, layers, dz)
        e32 = {k: float(np.abs(g - r.reshape(g.shape)).max() / np.abs(r).max())
               for k, g, r in zip(("z", "dx0", "slab"), got, ref)}
    xc, dc = (3, 2) if F % 2 else (0, 0)
    outs, pre, grid = _run_kernels(x, P, layers, dz, x_col0=xc, dx_col0=dc, pre_scale=float(np.abs(ddx).max()))
    assert grid == 1
    _assert_within("F=%d E=%d layers=%r B=1 live" % (F, E, layers), _errors(x, ref, outs[0], pre, grid, dc), e32,
                   _max_k(F, layers))


def test_cin_kernels_with_several_units_a_block(hip_lib):
    """B = 4,133 at (3, 8, (2,)): 1,034 units of 4 samples, past the forward's 1,024 blocks and the
    backward's 128 slab rows, so blocks take up to nine units in turn, reusing their LDS maps and adding
    the weight gradients into their slab row across them; the same bound."""
    F, E, layers, B = 3, 8, (2,), 4133
    x, P, dz, ref, _ = _reference(B, F, E, layers, 21)
    outs, pre, grid = _run_kernels(x, P, layers, dz, x_col0=3, dx_col0=2, runs=2, pre_scale=float(np.abs(ref[1]).max()))
    assert grid == 128
    for a, b in zip(outs[0], outs[1]):
        assert np.array_equal(_bits(a), _bits(b))
    _assert_within("F=%d E=%d layers=%r B=%d" % (F, E, layers, B), _errors(x, ref, outs[0], pre, grid, 2), None, 9)


def test_cin_kernels_refuse_what_they_cannot_take(hip_lib):
    t = torch.full((8, 2200), 3.0, device="cuda")
    prm = torch.zeros(8192, device="cuda")
    out = torch.full((64,), 3.0, device="cuda")
    slab = torch.full((8192,), 3.0, device="cuda")
    bad = [(1, 8, (2,)), (65, 8, (2,)), (4, 12, (2,)), (4, 8, ()), (4, 8, (2, 2, 2, 2)), (4, 8, (0,)), (4, 8, (65,)),
           (27, 8, (64, 64, 64)), (64, 8, (64, 2))]
    for F, E, h in bad:
        L, hl = len(h), _layers(h[:3])
        pat = "F %d fields|E %d not|L %d layers|H \\d+ feature maps|layer weights, more than" % (F, E, L)
        with pytest.raises(_lib.DLError, match=pat):
            call("dl_cin_fwd", 8, F, E, L, hl, ptr(t), 2200, 0, ptr(prm), None, ptr(out), _s())
        with pytest.raises(_lib.DLError, match=pat):
            call("dl_cin_bwd", 8, F, E, L, hl, ptr(t), 2200, 0, ptr(prm), ptr(out), ptr(t), 2200, 0, ptr(slab), 8, _s())
    hl = _layers((2,))
    with pytest.raises(_lib.DLError, match="field columns"):     # fields past x0's row
        call("dl_cin_fwd", 8, 4, 8, 1, hl, ptr(t), 2200, 2190, ptr(prm), None, ptr(out), _s())
    with pytest.raises(_lib.DLError, match="dx0 columns"):
        call("dl_cin_bwd", 8, 4, 8, 1, hl, ptr(t), 2200, 0, ptr(prm), ptr(out), ptr(t), 2200, 2190, ptr(slab), 8, _s())
    with pytest.raises(_lib.DLError, match="slab needs"):
        call("dl_cin_bwd", 8, 4, 8, 1, hl, ptr(t), 2200, 0, ptr(prm), ptr(out), ptr(t), 2200, 0, ptr(slab), 1, _s())
    torch.cuda.synchronize()
    assert (t == 3).all() and (out == 3).all() and (slab == 3).all()


# --------------------------------------------------------------------------- the engine: the shared bodies
# (tests/_side_options.py) on this option's row
@pytest.mark.parametrize("name", list(CIN.KW))
def test_trajectory_matches_restatement(hip_lib, name):
    trajectory_matches_restatement(CIN, name)


def test_with_the_whole_logit_chain(hip_lib):
    with_the(CIN, "the_whole_logit_chain")


def test_with_the_pooling_and_batch_norm(hip_lib):
    with_the(CIN, "the_pooling_and_batch_norm")


def test_with_the_product_layer(hip_lib):
    with_the(CIN, "the_product_layer")


def test_hidden_dropout_with_the_branch(hip_lib):
    follow(CIN, CIN.dropout)


def test_sample_weights_with_the_branch(hip_lib):
    follow(CIN, CIN.weighted)


def test_wrong_size_parameters_are_refused(hip_lib):
    wrong_size_parameters_are_refused(CIN)


@pytest.mark.parametrize("adam", ["dense", "lazy"])
def test_default_queues_the_kernels_it_queued(hip_lib, adam, monkeypatch):
    default_queues_the_kernels_it_queued(CIN, "dnn_pipeline", adam, monkeypatch)
