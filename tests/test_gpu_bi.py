"""GPU checks of the Bi-Interaction pooling (ModelSpec.bi_interaction, csrc/bi.hip):
dl_bi_fwd / dl_bi_bwd against the float64 closed forms (tests/_bi_ref.py); the engine with batch
normalisation (the NFM configuration) and its refusal of deep_0 at the other width.  The other engine-level
checks (trajectories, predict, checkpoint, export, local_run, the unchanged kernel sequence at
bi_interaction = False) are shared with the
other options: their bodies run on the "bi" row of tests/_side_options.py, called from the last section
here or collected as the [bi] cases of tests/test_gpu_side_options.py.

Kernel shapes (F, E): (2, 4) the smallest of both, one column group a sample; (3, 8) odd F; (26, 16) the
flagship's fields; (33, 8) one field past four unrolled loads of eight (and past eight of the backward's
four); (64, 32) the largest F; (5, 64) the largest E, 16 sample lanes a block; B = 1, 63, 300 (one
sample, a partial block, ten blocks of 32 samples with a partial last one).  The fields start at column
3 of x0 and q follows them, so these runs take the 4-B access form; the engine runs (column 0, pitches of
16 floats) and the aligned case below take the 16-B form."""
import numpy as np
import pytest
import torch

from deep_learning_amd import _lib
from deep_learning_amd._lib import call, ptr
from deep_learning_amd.engine import CTREngine, ModelSpec
from tests import _bi_ref as Bi
from tests._side_options import (BI, B_, MODES, TOL, _batches, _bits, _check, _engine, _init, _ref_run, _run, _s,
                                  default_queues_the_kernels_it_queued, follow, trajectory_matches_restatement,
                                  with_the)

pytestmark = pytest.mark.gpu

KW = BI.KW
SHAPES = [(2, 4), (3, 8), (26, 16), (33, 8), (64, 32), (5, 64)]


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


# --------------------------------------------------------------------------- 2. the engine, what only bi has
def test_wrong_width_parameters_are_refused(hip_lib):
    name = "dnn_cate"
    _, P0 = _init(BI, name, 1)
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
    _, P0 = _init(BI, name, 45, bn=True, jitter=0.2)
    bs = _batches(BI, name, 5, seed=13)
    zs, losses, P = _ref_run(BI, name, P0, bs, bn=True)
    for mode in ("atomic", "lazy"):
        eng = _engine(BI, name, spec=dict(batch_norm=True), init="none", **MODES[mode])
        eng.load_params({k: v.copy() for k, v in P0.items()})
        gz, gl = _run(eng, bs)
        _check(BI, eng, gz, gl, zs, losses, P, "nfm %s" % mode)


# --------------------------------------------------------------------------- the engine: the shared bodies
# (tests/_side_options.py) on this option's row
@pytest.mark.parametrize("name", list(BI.KW))
def test_trajectory_matches_restatement(hip_lib, name):
    trajectory_matches_restatement(BI, name)


def test_with_the_cross_network_and_the_attention(hip_lib):
    with_the(BI, "the_cross_network_and_the_attention")


def test_with_the_product_layer(hip_lib):
    with_the(BI, "the_product_layer")


def test_later_layer_dropout_with_the_pooling(hip_lib):
    follow(BI, BI.dropout)


def test_sample_weights_with_the_pooling(hip_lib):
    follow(BI, BI.weighted)


@pytest.mark.parametrize("adam", ["dense", "lazy"])
def test_default_queues_the_kernels_it_queued(hip_lib, adam, monkeypatch):
    default_queues_the_kernels_it_queued(BI, "dnn_pipeline", adam, monkeypatch)
