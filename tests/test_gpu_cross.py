"""GPU checks of the cross network (ModelSpec.cross_layers, csrc/cross.hip):
dl_cross_fwd / dl_cross_bwd against the float64 formulas (tests/_cross_ref.py) and the head's
z_extra twins.  The engine-level checks (trajectories, predict, checkpoint, export, local_run, the
unchanged kernel sequence at cross_layers = 0) are shared with the
other options: their bodies run on the "cross" row of tests/_side_options.py, called from the last section
here or collected as the [cross] cases of tests/test_gpu_side_options.py.

Kernel shapes: D = 37 (below a wave), 64 (one wave), 221 / 429 / 525 (ragged, 4 / 8 / 16 values
a lane with a partial last one), 1024 (the most); L = 1, 2, 4 (every register variant);
B = 1, 63 (a partial block), 300 (19 blocks of four waves: four passes of the grid)."""
import numpy as np
import pytest
import torch

from deep_learning_amd import _lib
from deep_learning_amd._lib import call, ptr
from tests import _cross_ref as X
from tests import _sample_weight_ref as W
from tests._side_options import (CROSS, TOL, _bits, _s, default_queues_the_kernels_it_queued, follow,
                                  trajectory_matches_restatement)

pytestmark = pytest.mark.gpu


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


# --------------------------------------------------------------------------- the engine: the shared bodies
# (tests/_side_options.py) on this option's row
@pytest.mark.parametrize("name", list(CROSS.KW))
def test_trajectory_matches_restatement(hip_lib, name):
    trajectory_matches_restatement(CROSS, name)


def test_hidden_dropout_with_the_cross(hip_lib):
    follow(CROSS, CROSS.dropout)


def test_sample_weights_with_the_cross(hip_lib):
    follow(CROSS, CROSS.weighted)


@pytest.mark.parametrize("adam", ["dense", "lazy"])
def test_default_queues_the_kernels_it_queued(hip_lib, adam, monkeypatch):
    default_queues_the_kernels_it_queued(CROSS, "dnn_pipeline", adam, monkeypatch)
