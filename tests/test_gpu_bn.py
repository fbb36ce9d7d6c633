"""GPU checks of batch normalisation in the deep tower (ModelSpec.batch_norm, csrc/bn.hip):
the dl_bn_* kernels against the float64 formulas (tests/_bn_ref.py); the engine with one Adam launch per
layer, a batch of one, predict on the running statistics and a poisoned step.  The other engine-level
checks (trajectories of one model of each family, checkpoint, export, local_run, the unchanged kernel
sequence at batch_norm off) are shared with the
other options: their bodies run on the "bn" row of tests/_side_options.py, called from the last section
here or collected as the [bn] cases of tests/test_gpu_side_options.py.

Kernel shapes (B, D): (2, 1) the smallest; (63, 33) odd sizes, a partial column group, two row blocks;
(300, 400) and (300, 416) the flagship's widths, a partial and a whole last halfword, ten row blocks;
(4099, 50) 129 row blocks, a short last one."""
import numpy as np
import pytest
import torch

from deep_learning_amd import _lib
from deep_learning_amd._lib import call, ptr
from deep_learning_amd.engine import CTREngine, ModelSpec
from oracle import ctr_ref as R
from tests import _bn_ref as Bn
from tests._side_options import (BN, B_, MODES, TOL, _batches, _bits, _check, _init, _run, _s,
                                  default_queues_the_kernels_it_queued, follow, trajectory,
                                  trajectory_matches_restatement, with_the)
from tests._side_options import _engine as _side_engine

pytestmark = pytest.mark.gpu

SHAPES = [(2, 1), (63, 33), (300, 400), (300, 416), (4099, 50)]
KW = BN.KW
FILL = -7.0


# --------------------------------------------------------------------------- 1. the kernels
def _run_kernels(fx, calls=1, with_bits=True, eps=Bn.EPS, m=Bn.MOMENTUM):
    """dl_bn_stats + dl_bn_fwd (`calls` times on a fresh C, the running statistics carried), then
    dl_bn_bwd_sums + dl_bn_bwd_apply.  Every matrix has a pitch above D and one row more than B, all
    pre-filled; returns the host copies."""
    c, gamma, beta, dy, rm, rv = fx
    B, D = c.shape
    Dp = (D + 15) // 16 * 16
    ldc, ldx, ldd, ldb = Dp + 4, Dp + 8, Dp + 12, (D + 15) // 16 + 2
    grid = _lib.lib().dl_bn_grid(B)

    def mat(v, ld):
        a = np.full((B + 1, ld), FILL, np.float32)
        a[:B, :D] = v
        return a
    c0, d0 = mat(c, ldc), mat(dy, ldd)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    par = dev(np.concatenate([gamma, beta]))
    run = dev(np.stack([rm, rv]))
    stat = torch.full((3 * Dp + 16,), FILL, device="cuda")
    ws = torch.zeros(_lib.lib().dl_bn_ws_floats(B, D), device="cuda")
    runs = []
    for _ in range(calls):
        C = dev(c0)
        hx = torch.full((B + 1, ldx), FILL, device="cuda")
        bits = torch.full((B + 1, ldb), 0x5555, dtype=torch.int16, device="cuda")
        call("dl_bn_stats", B, D, ptr(C), ldc, eps, m, ptr(stat), ptr(run[0]), ptr(run[1]), None, ptr(ws), ws.numel(),
             _s())
        call("dl_bn_fwd", B, D, ptr(C), ldc, ptr(stat), None, None, eps, ptr(par), ptr(hx), ldx,
             ptr(bits) if with_bits else None, ldb if with_bits else 0, _s())
        torch.cuda.synchronize()
        runs.append(run.cpu().numpy().copy())
    dyd = dev(d0)
    slab = torch.full((grid + 1, 2 * D), FILL, device="cuda")
    sums = torch.full((2 * Dp,), FILL, device="cuda")
    call("dl_bn_bwd_sums", B, D, ptr(dyd), ldd, ptr(hx), ldx, ptr(slab), grid, _s())
    call("dl_bn_bwd_apply", B, D, ptr(dyd), ldd, ptr(hx), ldx, ptr(par), ptr(stat), ptr(slab), grid, ptr(sums), _s())
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in dict(C=C, hx=hx, bits=bits, stat=stat, dc=dyd, slab=slab).items()}
    out.update(runs=runs, c0=c0, d0=d0, grid=grid, Dp=Dp)
    return out


@pytest.mark.parametrize("B,D", SHAPES)
def test_bn_kernels_match_fp64(hip_lib, B, D):
    """h, xhat, the saved mu and inverse standard deviation, the running statistics after one and after
    three calls, dc and the slab's column sums (dgamma, dbeta) within 1e-5 (absolute) of the float64
    formulas; the sign bits equal the reference's wherever its |gamma xhat + beta| > 1e-4 (at most 1 %
    left out, asserted on the reference) and equal h > 0 everywhere, zero bits past D, the halfwords past
    the row's, the columns past D and the row past B untouched; two runs give the same bits; without
    a bitmask h is the same.  Measured worst errors: DESIGN 4n."""
    fx = Bn.kernel_fixture(B, D, seed=1000 * D + B)
    c, gamma, beta, dy, rm, rv = fx
    ref = Bn.bn_fwd64(c, gamma, beta)
    dc64, dg64, db64 = Bn.bn_bwd64(dy, ref["xhat"], gamma, ref["invstd"])
    sure = np.abs(ref["y"]) > 1e-4
    assert sure.mean() >= 0.99
    assert B * D < 100 or 0.05 < (ref["y"] > 0).mean() < 0.95
    o, o2 = _run_kernels(fx, calls=3), _run_kernels(fx, calls=3)
    for k in ("C", "hx", "bits", "stat", "dc", "slab"):
        assert np.array_equal(o[k].view(np.uint8), o2[k].view(np.uint8)), k
    grid, Dp = o["grid"], o["Dp"]
    assert 1 <= grid <= 1024 and _lib.lib().dl_bn_grid(1 << 22) == 1024 and (B < 64 or grid > 1)
    for k, orig in (("C", o["c0"]), ("dc", o["d0"])):
        assert np.array_equal(_bits(o[k][B]), _bits(orig[B])) and np.array_equal(_bits(o[k][:, D:]), _bits(orig[:, D:])), k
    assert (o["hx"][B] == FILL).all() and (o["hx"][:, D:] == FILL).all()
    assert (o["slab"][grid] == FILL).all() and (o["stat"][3 * Dp:] == FILL).all()
    nh = (D + 15) // 16
    bg = o["bits"]
    assert (bg[B] == 0x5555).all() and (bg[:, nh:] == 0x5555).all()
    got_bits = ((bg[:B, :nh].astype(np.int32)[:, :, None] >> np.arange(16)) & 1).reshape(B, nh * 16)
    assert (got_bits[:, D:] == 0).all()
    assert np.array_equal(got_bits[:, :D][sure], (ref["y"] > 0)[sure].astype(np.int32))
    assert np.array_equal(got_bits[:, :D] == 1, o["C"][:B, :D] > 0)
    st = o["stat"].astype(np.float64)
    run1 = Bn.running_update(rm, rv, ref["mu"], ref["var"], B)
    run3 = run1
    for _ in range(2):
        run3 = Bn.running_update(run3[0], run3[1], ref["mu"], ref["var"], B)
    err = dict(h=np.abs(o["C"][:B, :D] - ref["h"]).max(), xhat=np.abs(o["hx"][:B, :D] - ref["xhat"]).max(),
               mu=np.abs(st[:D] + st[Dp:Dp + D] - ref["mu"]).max(), invstd=np.abs(st[2 * Dp:2 * Dp + D] - ref["invstd"]).max(),
               run1=max(np.abs(o["runs"][0][i] - run1[i]).max() for i in (0, 1)),
               run3=max(np.abs(o["runs"][2][i] - run3[i]).max() for i in (0, 1)),
               dc=np.abs(o["dc"][:B, :D] - dc64).max(),
               dgamma=np.abs(o["slab"][:grid, :D].astype(np.float64).sum(0) - dg64).max(),
               dbeta=np.abs(o["slab"][:grid, D:].astype(np.float64).sum(0) - db64).max())
    print("max |kernel - fp64| (B %d, D %d):" % (B, D), {k: float(v) for k, v in err.items()})
    for k, v in err.items():
        assert v < TOL, (k, v)
    nb = _run_kernels(fx, with_bits=False)
    one = _run_kernels(fx)
    assert np.array_equal(_bits(nb["C"]), _bits(one["C"])) and (nb["bits"] == 0x5555).all()


def test_cancellation_keeps_xhat(hip_lib):
    """The (300, 400) case with 1,000 added to every column (std still in [0.25, 4]): xhat within 1e-5
    (absolute) of (c - mu) invstd in float64 on the f32-rounded c.  A raw-moment variance misses this by
    orders of magnitude (tests/test_bn_cpu.py shows both forms in float32)."""
    fx = Bn.kernel_fixture(300, 400, 77, offset=1000.0)
    ref = Bn.bn_fwd64(fx[0], fx[1], fx[2])
    o = _run_kernels(fx)
    err = np.abs(o["hx"][:300, :400] - ref["xhat"]).max()
    print("cancellation: max |xhat - fp64| =", float(err))
    assert err < TOL
    assert np.abs(o["C"][:300, :400] - ref["h"]).max() < TOL


def test_constant_columns(hip_lib):
    """Columns that are 0.5 in every row (B = 300: the f32 sums are exact): xhat = 0 exactly and
    h = relu(beta) exactly, everything finite.  The issue's dc = gamma invstd (dy - dbeta / B - xhat
    dgamma / B) is gamma / sqrt(eps) (dy - mean dy) there: exactly 0 in column 3, whose dy is one
    value in every row, and the closed form (torch's, too) in column 5, whose dy varies."""
    B, D = 300, 48
    c, gamma, beta, dy, rm, rv = Bn.kernel_fixture(B, D, 5)
    c[:, [3, 5]] = 0.5
    dy[:, 3] = 0.25
    ref = Bn.bn_fwd64(c, gamma, beta)
    dc64, _, _ = Bn.bn_bwd64(dy, ref["xhat"], gamma, ref["invstd"])
    o = _run_kernels((c, gamma, beta, dy, rm, rv))
    for k in ("C", "hx", "dc", "stat", "slab"):
        assert np.isfinite(o[k]).all(), k
    for j in (3, 5):
        assert (o["hx"][:B, j] == 0).all()
        assert np.array_equal(_bits(o["C"][:B, j]), _bits(np.full(B, max(beta[j], 0), np.float32)))
    assert (o["dc"][:B, 3] == 0).all()
    assert np.abs(o["dc"][:B, :D] - dc64).max() < TOL and np.abs(dc64[:, 5]).max() > 0.1


def test_inference_mode(hip_lib):
    """dl_bn_fwd without stat normalises by the given running statistics (bn_fwd64's eval mode) and
    leaves them alone; hx is refused there."""
    for B, D in ((1, 33), (300, 400)):
        c, gamma, beta, _, rm, rv = Bn.kernel_fixture(B, D, 9)
        ref = Bn.bn_fwd64(c, gamma, beta, running=(rm, rv))
        ldc = (D + 15) // 16 * 16 + 4
        c0 = np.full((B + 1, ldc), FILL, np.float32)
        c0[:B, :D] = c
        C = torch.from_numpy(c0).cuda()
        par = torch.from_numpy(np.concatenate([gamma, beta])).cuda()
        run = torch.from_numpy(np.stack([rm, rv])).cuda()
        bits = torch.zeros((B, (D + 15) // 16), dtype=torch.int16, device="cuda")
        call("dl_bn_fwd", B, D, ptr(C), ldc, None, ptr(run[0]), ptr(run[1]), Bn.EPS, ptr(par), None, 0, ptr(bits),
             bits.shape[1], _s())
        torch.cuda.synchronize()
        got = C.cpu().numpy()
        assert np.abs(got[:B, :D] - ref["h"]).max() < TOL
        assert np.array_equal(_bits(got[:, D:]), _bits(c0[:, D:])) and np.array_equal(_bits(got[B]), _bits(c0[B]))
        assert np.array_equal(run.cpu().numpy(), np.stack([rm, rv]))
        gb = ((bits.cpu().numpy().astype(np.int32)[:, :, None] >> np.arange(16)) & 1).reshape(B, -1)[:, :D]
        assert np.array_equal(gb == 1, got[:B, :D] > 0)
        with pytest.raises(_lib.DLError, match="no hx"):
            call("dl_bn_fwd", B, D, ptr(C), ldc, None, ptr(run[0]), ptr(run[1]), Bn.EPS, ptr(par), ptr(C), ldc, None, 0, _s())


def test_bn_kernels_refuse_what_they_cannot_take(hip_lib):
    t = torch.full((8, 64), 3.0, device="cuda")
    u = torch.full((8, 64), 3.0, device="cuda")
    small = torch.full((4096,), 3.0, device="cuda")
    n = small.numel()
    st = lambda B, D, ld: call("dl_bn_stats", B, D, ptr(t), ld, 1e-5, 0.1, ptr(small), None, None, None, ptr(small), n, _s())
    for B, D, ld, msg in ((8, 0, 64, "D 0 < 1"), (1, 4, 64, "B 1 < 2"), (8, 40, 36, "ldc 36"), (8, 4, 6, "ldc 6")):
        with pytest.raises(_lib.DLError, match=msg):
            st(B, D, ld)
    with pytest.raises(_lib.DLError, match="ws needs"):
        call("dl_bn_stats", 8, 4, ptr(t), 64, 1e-5, 0.1, ptr(small), None, None, None, ptr(small), 8, _s())
    with pytest.raises(_lib.DLError, match="D 0 < 1"):
        call("dl_bn_fwd", 8, 0, ptr(t), 64, ptr(small), None, None, 1e-5, ptr(small), ptr(u), 64, None, 0, _s())
    with pytest.raises(_lib.DLError, match="ldx 36"):
        call("dl_bn_fwd", 8, 40, ptr(t), 64, ptr(small), None, None, 1e-5, ptr(small), ptr(u), 36, None, 0, _s())
    with pytest.raises(_lib.DLError, match="ldbits"):
        call("dl_bn_fwd", 8, 40, ptr(t), 64, ptr(small), None, None, 1e-5, ptr(small), ptr(u), 64, ptr(small), 2, _s())
    for B, D, msg in ((1, 4, "B 1 < 2"), (8, 0, "D 0 < 1")):
        with pytest.raises(_lib.DLError, match=msg):
            call("dl_bn_bwd_sums", B, D, ptr(t), 64, ptr(u), 64, ptr(small), 1, _s())
        with pytest.raises(_lib.DLError, match=msg):
            call("dl_bn_bwd_apply", B, D, ptr(t), 64, ptr(u), 64, ptr(small), ptr(small), ptr(small), 1, ptr(small), _s())
    with pytest.raises(_lib.DLError, match="slab needs"):
        call("dl_bn_bwd_sums", 64, 4, ptr(t), 64, ptr(u), 64, ptr(small), 1, _s())
    torch.cuda.synchronize()
    assert (t == 3).all() and (u == 3).all() and (small == 3).all()


# --------------------------------------------------------------------------- 2. the engine, what only bn has
def _engine(name, P0, mode="lazy", **spec_kw):
    sw = spec_kw.pop("sample_weight", False)
    eng = _side_engine(BN, name, spec=spec_kw, init="none", sample_weight=sw, **MODES[mode])
    eng.load_params({k: v.copy() for k, v in P0.items()})
    return eng


def test_one_adam_launch_per_layer(hip_lib, monkeypatch):
    monkeypatch.setenv("DLAMD_ADAM_FUSED", "0")
    name = "dnn_pipeline"
    P0, bs, zs, losses, P = trajectory(BN, name)
    eng = _engine(name, P0)
    assert not eng._adam_fused()
    gz, gl = _run(eng, bs)
    _check(BN, eng, gz, gl, zs, losses, P, "adam per layer")


def test_batch_of_one_is_refused_before_anything_is_queued(hip_lib, monkeypatch):
    from deep_learning_amd import engine as E
    name = "dnn_pipeline"
    eng = CTREngine(ModelSpec(name, batch_norm=True, **KW[name]), max_batch=B_, seed=3)
    b = {k: v[:1] for k, v in _batches(BN, name, 1)[0].items()}
    names = []
    real = E.call
    monkeypatch.setattr(E, "call", lambda n, *a: (names.append(n), real(n, *a))[1])
    with pytest.raises(ValueError, match="batch_norm: a training batch needs at least 2 samples"):
        eng.train_step(b)
    assert not names and eng.steps == 0
    assert eng.predict(b).shape == (1,)


def test_predict_uses_the_running_statistics(hip_lib):
    """After training, predict equals the restatement in eval mode within 1e-5 and differs from a
    train-mode forward on the same batch by more than 1e-3; lazy tables: predict after training, after
    flush() and on flush(planes=True)'s planes (unfused: layer 0 stores its pre-activation) agree bit
    for bit."""
    name = "dnn_pipeline"
    _, P0 = _init(BN, name, 9)
    eng = _engine(name, P0)
    bs = _batches(BN, name, 6, seed=40)
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
    cfg = R.make_cfg(name, **KW[name])
    P = eng.params()
    ev = Bn.forward_backward(cfg, P, b, bn=True, train=False)
    tr = Bn.forward_backward(cfg, P, b, bn=True, train=True)
    assert np.abs(z0 - ev["z"]).max() < TOL
    assert np.abs(z0 - tr["z"]).max() > 1e-3
    run = {k: v for k, v in P.items() if "running" in k}
    after = eng.params()
    for k in run:       # predict leaves the running statistics alone
        np.testing.assert_array_equal(run[k], after[k])


def test_poisoned_step_leaves_the_layer_alone(hip_lib):
    """A batch with an out-of-range id: gamma, beta, their moments and the running statistics keep
    their bits; the next batch applies normally."""
    name = "dnn_pipeline"
    _, P0 = _init(BN, name, 12)
    for mode in ("atomic", "lazy"):
        eng = _engine(name, P0, mode)
        bs = _batches(BN, name, 3, seed=80)
        eng.train_step(bs[0])
        torch.cuda.synchronize()
        eng.check_error()
        keys = [k for k in eng.params() if k.startswith("batch_norm")]
        state = lambda: ({k: eng.params()[k] for k in keys}, eng.dense_state())
        p1, s1 = state()
        bad = {k: np.array(v, copy=True) for k, v in bs[1].items()}
        bad["cate_feats"][5, 2] = KW[name]["cate_index_size"] + 7
        raised = []
        for step in (lambda: eng.train_step(bad), torch.cuda.synchronize, eng.check_error):
            try:
                step()                                 # (the batch's step is issued even if train_step raises)
            except _lib.DLError as e:
                raised.append(str(e))
        assert len(raised) == 1 and "out of range" in raised[0], raised
        p2, s2 = state()
        for k in keys:
            np.testing.assert_array_equal(p1[k], p2[k], err_msg=k)
        for mv in ("m", "v"):
            for k in keys:
                if "running" not in k:
                    np.testing.assert_array_equal(s1[mv][k], s2[mv][k], err_msg=k)
        eng.train_step(bs[2])
        torch.cuda.synchronize()
        eng.check_error()
        p3, _ = state()
        assert all(np.abs(p3[k] - p2[k]).max() > 0 for k in keys)


# --------------------------------------------------------------------------- the engine: the shared bodies
# (tests/_side_options.py) on this option's row
@pytest.mark.parametrize("name", list(BN.KW))
def test_trajectory_matches_restatement(hip_lib, name):
    trajectory_matches_restatement(BN, name)


def test_with_the_cross_network_and_the_attention(hip_lib):
    with_the(BN, "the_cross_network_and_the_attention")


def test_sample_weights(hip_lib):
    follow(BN, BN.weighted)


@pytest.mark.parametrize("name,adam", BN.defaults)
def test_default_queues_the_kernels_it_queued(hip_lib, name, adam, monkeypatch):
    default_queues_the_kernels_it_queued(BN, name, adam, monkeypatch)
