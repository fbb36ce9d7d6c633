"""GPU checks of sample weighting (include/dlamd.h "Sample weights"): dl_weight_norm bit
for bit against numpy; the four *_weighted head entry points against the float64 restatement
(tests/_sample_weight_ref.py); the engine bit-identical to the plain one for unit weights; weighted
trajectories against the oracle's Adam; zero weights; a bad weight skipped alone; the weight slots
double-buffered with the prefetch; eval_stats(weights=) and CTRModel.eval with weight_key.

Shapes: S = 8, E = 16, hidden [48, 32], a few thousand rows; B = 1, 67 (no multiple of the wave or
the heads' look-ahead), 300 (several head blocks, a partial last round), 2500 (dl_weight_norm: more
than its block's 1024 threads, a partial second round)."""
import types

import numpy as np
import pytest
import torch

from deep_learning_amd import _lib, metrics
from deep_learning_amd._lib import call, ptr
from deep_learning_amd.engine import CTREngine, ModelSpec
from deep_learning_amd.synthetic import make_batch
from oracle import ctr_ref as R
from tests import _dropout_ref as D
from tests import _sample_weight_ref as W

pytestmark = pytest.mark.gpu

TOL = 1e-5
PW = 2.5
KW = {"deepfm_pipeline": dict(C=13, S=8, E=16, cate_index_size=4000, hidden=[48, 32]),
      "dnn_cate": dict(V=3, S=8, E=16, cate_index_size=4000, hidden=[48, 32]),
      "wdl": dict(C=13, S=8, E=16, cate_index_size=4000, hidden=[48, 32], Fw=8)}


def _s():
    return _lib.stream_handle()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _rel(got, ref):
    """max |got - ref| over the array's largest reference magnitude: the 1e-5 bar's measure."""
    ref = np.asarray(ref, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / max(np.abs(ref).max(), 1e-30))


def _weights(B, seed):
    return np.random.default_rng(seed).choice(np.float32([0, 0.5, 1, 3]), B).astype(np.float32)


# --------------------------------------------------------------------------- 1. dl_weight_norm
def _weight_norm(weight, label, pw):
    B = label.size
    y = torch.from_numpy(label).cuda()
    w = None if weight is None else torch.from_numpy(weight).cuda()
    we = torch.full((B + 8,), -7.0, device="cuda")
    norm = torch.full((4,), -7.0, device="cuda")
    err = torch.zeros(4, dtype=torch.int32, device="cuda")
    call("dl_weight_norm", ptr(w), ptr(y), B, pw, ptr(we), ptr(norm), ptr(err), _s())
    torch.cuda.synchronize()
    return we.cpu().numpy(), norm.cpu().numpy(), err.cpu().numpy()


@pytest.mark.parametrize("B", [1, 67, 300, 2500])
def test_weight_norm_bits(hip_lib, B):
    """w_eff, N_nz and inv_norm bit for bit for random weights, a NULL weight pointer (all ones:
    inv_norm is the f32 of 1 / B) and all-zero weights (inv_norm 0); nothing past B is written and
    the validation word stays clear.  A negative, a NaN and an infinite weight each set
    DL_STATUS_BAD_WEIGHT and nothing else, and that sample's w_eff is 0."""
    rng = np.random.default_rng(B)
    y = (rng.random(B) < 0.3).astype(np.float32)
    if B > 1:
        y[:2] = [1, 0]
    for weight, pw in ((_weights(B, 1), PW), (None, 1.0), (None, 0.3), (np.zeros(B, np.float32), PW),
                       (rng.random(B).astype(np.float32), 1.7)):
        we, norm, err = _weight_norm(weight, y, pw)
        want, nz, inv, bad = W.w_eff_f32(weight, y, pw)
        assert not bad and not err.any()
        assert np.array_equal(_bits(we[:B]), _bits(want)) and (we[B:] == -7).all()
        assert norm[1] == nz and _bits(norm[:1])[0] == _bits(np.float32([inv]))[0] and (norm[2:] == -7).all()
        if weight is None and pw == 1.0:
            assert nz == B and norm[0] == np.float32(1.0 / B)
    assert _weight_norm(np.zeros(B, np.float32), y, PW)[1][0] == 0
    for v in (-0.5, np.nan, np.inf):
        weight = _weights(B, 2)
        weight[B // 2] = v
        we, norm, err = _weight_norm(weight, y, PW)
        want, nz, inv, bad = W.w_eff_f32(weight, y, PW)
        assert bad and list(err) == [_lib.STATUS_BAD_WEIGHT, 0, 0, 0]
        assert np.array_equal(_bits(we[:B]), _bits(want)) and we[B // 2] == 0 and norm[1] == nz


# --------------------------------------------------------------------------- 2. the weighted heads
def _norm_dev(w):
    nz, _ = W.norm64(w)
    return torch.tensor([np.float32(1.0 / nz) if nz else 0.0, float(nz)], dtype=torch.float32).cuda()


def _fm_head(B, drop):
    """dl_head_fwd_bwd[_fmdrop]_weighted on random inputs; returns (outputs, float64 reference)."""
    g = torch.Generator().manual_seed(23 + B)
    F, E, H = 21, 16, 32
    fm_cols, fm_ld, ldh = F + E, F + E + 3, H + 4
    fm = torch.randn(B, fm_ld, generator=g)
    h = torch.relu(torch.randn(B, ldh, generator=g))
    w = torch.randn(fm_cols + H + 1, generator=g) * 0.1
    y = (torch.rand(B, generator=g) < 0.3).float()
    we = torch.from_numpy(W.w_eff_f32(_weights(B, 5), y.numpy(), PW)[0])
    grid = _lib.lib().dl_head_grid(B)
    out = {k: v.cuda() for k, v in dict(score=torch.zeros(B), z=torch.zeros(B), dz=torch.zeros(B),
                                        dh=torch.zeros(B, ldh), slab=torch.zeros(grid, fm_cols + H + 2)).items()}
    dev = [t.cuda() for t in (fm, h, w, y, we)] + [_norm_dev(we.numpy())]
    args = [B, fm_cols, H, ptr(dev[0]), fm_ld, ptr(dev[1]), ldh, ptr(dev[2]), ptr(dev[3]), 1e-7, ptr(dev[4]),
            ptr(dev[5]), ptr(out["score"]), ptr(out["z"]), ptr(out["dz"]), ptr(out["dh"]),
            ptr(out["slab"]), grid]
    feat_fm = fm[:, :fm_cols].numpy().astype(np.float64)
    if drop:
        from tests import _fm_dropout_ref as FD
        keeps, seed, step = (0.7, 0.6), 2019 + (7 << 32), 5
        opt = torch.zeros(_lib.OPT_LEN)
        opt[7] = step
        opt = opt.cuda()
        keep = torch.zeros(B, 2, dtype=torch.int64, device="cuda")
        call("dl_head_fwd_bwd_fmdrop_weighted", *args, F, D.keep_thr(keeps[0]), float(D.inv_keep(keeps[0])),
             D.keep_thr(keeps[1]), float(D.inv_keep(keeps[1])), seed, ptr(opt), ptr(keep), _s())
        m1, m2 = FD.fm_masks(seed, step, B, F, E, keeps)
        scale = np.concatenate([np.where(m1, D.inv_keep(keeps[0]), np.float32(0)),
                                np.where(m2, D.inv_keep(keeps[1]), np.float32(0))], 1).astype(np.float32)
        feat_fm = (fm[:, :fm_cols].numpy() * scale).astype(np.float64)
    else:
        call("dl_head_fwd_bwd_weighted", *args, _s())
    torch.cuda.synchronize()
    hh = h[:, :H].numpy().astype(np.float64)
    ref = W.head64(np.concatenate([feat_fm, hh], 1), w[:-1].numpy(), float(w[-1]), y.numpy(), we.numpy())
    ref["dh"] = ref["dfeat"][:, fm_cols:] * (hh > 0)
    ref["slab"] = np.concatenate([ref["dw"], [ref["db"]]])
    ref["lsum"] = float((we.numpy().astype(np.float64) * W.per_sample_loss(ref["p"], y.numpy(), 1e-7)).sum())
    got = {k: v.cpu().numpy() for k, v in out.items()}
    got["dh"] = got["dh"][:, :H]
    return got, ref, we.numpy()


def _check_head(got, ref, we, dh_tol=None):
    slab = got["slab"].astype(np.float64).sum(0)
    err = dict(score=_rel(got["score"], ref["p"]), z=_rel(got["z"], ref["z"]), dz=_rel(got["dz"], ref["dz"]),
               slab=_rel(slab[:-1], ref["slab"]), loss=abs(slab[-1] - ref["lsum"]) / max(abs(ref["lsum"]), 1e-30))
    if dh_tol is None:
        err["dh"] = _rel(got["dh"], ref["dh"])
    print("max relative error:", err)
    for k, v in err.items():
        assert v < TOL, (k, v)
    assert (got["dz"][we == 0] == 0).all()
    if dh_tol is not None:      # bf16 dh: half an ulp of the format is 2^-9 relative; 2^-8 allowed
        d = np.abs(got["dh"].astype(np.float64) - ref["dh"])
        assert (d <= dh_tol * np.abs(ref["dh"]) + TOL * np.abs(ref["dh"]).max()).all()


@pytest.mark.parametrize("drop", [False, True], ids=["plain", "fmdrop"])
@pytest.mark.parametrize("B", [1, 67, 300])
def test_fm_head_weighted_matches_fp64(hip_lib, B, drop):
    """score, z, dz, dh, the slab's column sums and its loss column against the float64
    restatement, each within 1e-5 of the array's largest magnitude; zero-weight samples get dz == 0
    exactly.  Measured worst over the six cases (printed): z 2.6e-7, dz 2.0e-7, slab 1.9e-7, dh 1.7e-7,
    loss column 8.2e-8, score 9.0e-8."""
    _check_head(*_fm_head(B, drop))


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("B", [1, 67, 300])
def test_wdl_head_weighted_matches_fp64(hip_lib, B, bf16):
    """dl_wdl_head_fwd_bwd[_bf16]_weighted: as the FM head's check, the wide rows' fixed-point
    gradient included; the bf16 dh within the format's rounding (2^-8 relative) of the reference.
    Measured worst (printed): z 7.6e-8, dz 1.9e-7, slab 2.3e-7, dh (f32) 1.6e-7, loss column 1.3e-7,
    wide gradient 2.1e-7."""
    g = torch.Generator().manual_seed(41 + B)
    Fw, H, rows = 8, 32, 500
    ldh = H + 16
    h = torch.relu(torch.randn(B, ldh, generator=g))
    w = torch.randn(rows, generator=g) * 0.1
    bias = torch.tensor([0.05, 0, 0, 0])
    wide = torch.randint(0, rows, (B, Fw), generator=g)
    y = (torch.rand(B, generator=g) < 0.3).float()
    we = W.w_eff_f32(_weights(B, 6), y.numpy(), PW)[0]
    grid = _lib.lib().dl_wdl_head_grid(B)
    out = {k: v.cuda() for k, v in dict(score=torch.zeros(B), z=torch.zeros(B), dz=torch.zeros(B),
                                        slab=torch.zeros(grid, H + 2)).items()}
    dh = torch.zeros(B, ldh, dtype=torch.bfloat16 if bf16 else torch.float32, device="cuda")
    gw = torch.zeros(rows, dtype=torch.int64, device="cuda")
    touched = torch.zeros(rows, dtype=torch.uint8, device="cuda")
    err = torch.zeros(4, dtype=torch.int32, device="cuda")
    dev = [t.cuda() for t in (wide, h, w, bias, y, torch.from_numpy(we))] + [_norm_dev(we)]
    call("dl_wdl_head_fwd_bwd_bf16_weighted" if bf16 else "dl_wdl_head_fwd_bwd_weighted", B, Fw, H, ptr(dev[0]), Fw,
         ptr(dev[1]), ldh, ptr(dev[2]), ptr(dev[3]), rows, ptr(dev[4]), 1e-7, ptr(dev[5]), ptr(dev[6]),
         ptr(out["score"]), ptr(out["z"]), ptr(out["dz"]), ptr(dh), ptr(gw), ptr(touched), ptr(out["slab"]), grid,
         ptr(err), _s())
    torch.cuda.synchronize()
    assert not err.cpu().numpy().any()
    hh = h[:, :H].numpy().astype(np.float64)
    w64 = w.numpy().astype(np.float64)
    feat = np.concatenate([np.ones((B, Fw)), hh], 1)
    z = w64[wide.numpy()].sum(1) + hh @ w64[Fw:Fw + H] + 0.05
    p = 1 / (1 + np.exp(-z))
    dz = W.dz64(p, y.numpy(), we)
    gwide = np.zeros(rows)
    np.add.at(gwide, wide.numpy().reshape(-1), np.repeat(dz, Fw))
    ref = dict(z=z, p=p, dz=dz, dh=dz[:, None] * w64[None, Fw:Fw + H] * (hh > 0),
               slab=np.concatenate([hh.T @ dz, [dz.sum()]]),
               lsum=float((we.astype(np.float64) * W.per_sample_loss(p, y.numpy(), 1e-7)).sum()))
    assert feat.shape[1] == Fw + H
    got = {k: v.cpu().numpy() for k, v in out.items()}
    got["dh"] = dh.float().cpu().numpy()[:, :H]
    _check_head(got, ref, we, dh_tol=2.0 ** -8 if bf16 else None)
    e = _rel(gw.cpu().numpy() / _lib.WIDE_GRAD_SCALE, gwide)
    print("wide gradient:", e)
    assert e < TOL


# --------------------------------------------------------------------------- engines
def _batches(name, B, n, seed=11, weights=True):
    kw = KW[name]
    out = []
    for i in range(n):
        C = kw.get("C", 0)
        b = make_batch(B, cont=C, vector=kw.get("V", 0), cate_fields=kw["S"], cate_index_size=kw["cate_index_size"],
                       seed=seed + i, wide_fields=kw.get("Fw", 0), cate_only=C == 0)
        if B > 1:
            b["cate_feats"][0, :2] = [0, 1]
        if weights:
            b["weight"] = _weights(B, seed + 50 + i).reshape(B, 1)
        out.append(b)
    return out


def _run(eng, bs, graph, prefetch=False):
    zs, losses = [], []
    for i, b in enumerate(bs):
        nxt = bs[i + 1] if prefetch and i + 1 < len(bs) else None
        eng.train_step(b, graph=graph, next_batch=nxt)
        torch.cuda.synchronize()
        zs.append(eng.z[: eng.last_batch].cpu().numpy().copy())
        losses.append(eng.loss())
    eng.check_error()
    return zs, losses


def _same(a, b):
    pa, pb = a.params(), b.params()
    for k in pa:
        np.testing.assert_array_equal(pa[k], pb[k], err_msg=k)


# --------------------------------------------------------------------------- 3. bit-identity
@pytest.mark.parametrize("name,adam", [("deepfm_pipeline", "lazy"), ("dnn_cate", "dense"), ("wdl", "lazy"),
                                       ("wdl", "dense")])
def test_unit_weights_are_the_plain_engine(hip_lib, name, adam):
    """sample_weight=True fed all-ones weights (given, and left out of the batch), and pos_weight=1.0,
    against the plain engine over 4 graph steps: logits, loss, the running loss sum and every
    parameter (the whole tables) bit for bit.  The plain engine holds none of the new buffers."""
    B = 300
    bs = _batches(name, B, 4, weights=False)
    ones = [dict(b, weight=np.ones((B, 1), np.float32)) for b in bs]
    mk = lambda pw=None, **e: CTREngine(ModelSpec(name, **KW[name], **({} if pw is None else {"pos_weight": pw})),
                                        max_batch=B, seed=5, adam=adam, **e,
                                        **({} if adam == "lazy" else {"bwd": "sorted"}))   # atomic: order varies
    plain, pw1, sw, sw_nokey = mk(), mk(1.0), mk(sample_weight=True), mk(sample_weight=True)
    for e in (plain, pw1):
        assert not e.weighted and not any(hasattr(e, a) for a in ("in_weight", "w_eff", "norm"))
    assert sw.weighted and {"in_weight", "w_eff", "norm"} <= set(CTREngine.SLOT_ATTRS)
    res = []
    for eng, data in ((plain, bs), (pw1, bs), (sw, ones), (sw_nokey, bs)):
        eng.loss_sum_begin()
        zs, losses = _run(eng, data, graph=True)
        res.append((zs, losses, eng.loss_sum_end()))
    for zs, losses, total in res[1:]:
        for a, b in zip(zs, res[0][0]):
            np.testing.assert_array_equal(a, b)
        assert losses == res[0][1] and total == res[0][2]
    for e in (pw1, sw, sw_nokey):
        _same(plain, e)
    assert float(sw.norm[1].item()) == B


# --------------------------------------------------------------------------- 4. trajectories
@pytest.fixture(scope="module")
def trajectories():
    """The oracle's 5 weighted steps (weights in {0, 0.5, 1, 3}, pos_weight 2.5), once per model."""
    out = {}
    for name in ("deepfm_pipeline", "wdl"):
        cfg = R.make_cfg(name, **KW[name])
        P0 = R.init_params(cfg, np.random.default_rng(42))
        P = {k: v.copy() for k, v in P0.items()}
        opt = R.AdamTF1(cfg, P)
        bs = _batches(name, 300, 5)
        fws = [W.train_step(cfg, P, opt, b, PW) for b in bs]
        out[name] = (P0, bs, [f["z"] for f in fws], [f["loss"] for f in fws], P)
    return out


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("name", ["deepfm_pipeline", "wdl"])
def test_weighted_trajectory_matches_oracle(hip_lib, trajectories, name, graph):
    """5 weighted steps, lazy and dense(sorted) tables: logits, every step's loss() and the final
    parameters within 1e-5 of the reference helper driving the oracle's Adam; loss_sum_end() is the
    sum of the loss() values (1e-5 a step); lazy and dense bit-identical to each other."""
    P0, bs, zs, losses, P = trajectories[name]
    engs = []
    for ekw in ({"adam": "lazy"}, {"bwd": "sorted"}):
        eng = CTREngine(ModelSpec(name, pos_weight=PW, **KW[name]), max_batch=300, init="none", sample_weight=True,
                        **ekw)
        eng.load_params({k: v.copy() for k, v in P0.items()})
        eng.loss_sum_begin()
        gz, gl = _run(eng, bs, graph)
        total, steps = eng.loss_sum_end()
        err = dict(z=max(np.abs(a - b).max() for a, b in zip(gz, zs)),
                   loss=max(abs(a - b) for a, b in zip(gl, losses)), sum=abs(total - sum(gl)))
        got = eng.params()
        err["params"] = max(np.abs(got[k] - P[k]).max() for k in P)
        print(name, ekw, "max |engine - oracle|:", {k: float(v) for k, v in err.items()})
        assert steps == 5 and err["sum"] < TOL * 5
        for k in ("z", "loss", "params"):
            assert err[k] < TOL, (k, err[k])
        engs.append((eng, gz, gl))
    for a, b in zip(engs[0][1], engs[1][1]):
        np.testing.assert_array_equal(a, b)
    _same(engs[0][0], engs[1][0])
    plain = CTREngine(ModelSpec(name, **KW[name]), max_batch=300, init="none", adam="lazy")
    plain.load_params({k: v.copy() for k, v in P0.items()})
    _run(plain, bs[:2], graph)
    assert np.abs(plain.z[:300].cpu().numpy() - zs[1]).max() > 10 * TOL      # the weights do matter


# --------------------------------------------------------------------------- 5. zero weights
@pytest.mark.parametrize("name", ["deepfm_pipeline", "wdl"])
def test_zero_weights(hip_lib, name):
    """All weights zero: loss() is the regulariser term alone, dz is all zero, and the parameters
    move exactly as in a step whose data gradient is zero (a twin fed other labels and features'
    weights, also all zero, ends with the same bits).  k zero weights among B: those dz are 0."""
    B = 67
    cfg = R.make_cfg(name, **KW[name])
    P0 = R.init_params(cfg, np.random.default_rng(1))
    b0, b1, b2 = _batches(name, B, 3)
    mk = lambda: CTREngine(ModelSpec(name, **KW[name]), max_batch=B, init="none", adam="lazy", sample_weight=True)
    eng, twin = mk(), mk()
    for e in (eng, twin):
        e.load_params({k: v.copy() for k, v in P0.items()})
        e.train_step(b0)                     # nonzero moments: the zero-gradient step still moves rows
    zero = dict(b1, weight=np.zeros((B, 1), np.float32))
    eng.train_step(zero)
    torch.cuda.synchronize()
    assert not eng.dz[:B].cpu().numpy().any() and float(eng.norm[0].item()) == 0
    P1 = {k: v.copy() for k, v in P0.items()}
    W.train_step(cfg, P1, R.AdamTF1(cfg, P1), b0)
    assert abs(eng.loss() - R._reg_loss(cfg, P1)) < TOL and R._reg_loss(cfg, P1) > 0
    flipped = dict(zero, label=1 - b1["label"])
    twin.train_step(flipped)                 # same ids (same rows touched), other labels: same zero gradient
    torch.cuda.synchronize()
    _same(eng, twin)
    eng.train_step(b2)
    torch.cuda.synchronize()
    eng.check_error()
    k = b2["weight"].reshape(-1) == 0
    dz = eng.dz[:B].cpu().numpy()
    assert 0 < k.sum() < B and (dz[k] == 0).all() and (dz[~k] != 0).all()


# --------------------------------------------------------------------------- 6. bad weight
@pytest.mark.parametrize("name,adam", [("deepfm_pipeline", "lazy"), ("wdl", "dense")])
def test_bad_weight_batch_skipped_alone_and_raises(hip_lib, name, adam):
    """A batch with a negative weight applies nothing and raises within two calls, naming the
    weight and the global step skipped; the batches around it train: the final state is an engine's
    that never saw it, bit for bit (as test_bad_id_batch_skipped_alone_and_raises)."""
    B = 67
    mk = lambda: CTREngine(ModelSpec(name, pos_weight=PW, **KW[name]), max_batch=B, seed=4, adam=adam,
                           **({} if adam == "lazy" else {"bwd": "sorted"}))
    eng, twin = mk(), mk()
    bs = _batches(name, B, 6, seed=13)
    bad = {k: v.copy() for k, v in bs[3].items()}
    bad["weight"][9] = -1.0
    raised = []
    for i, b in enumerate(bs[:3] + [bad] + bs[4:]):
        try:
            eng.train_step(b, graph=i >= 1)
        except _lib.DLError as e:
            raised.append(str(e))
    torch.cuda.synchronize()
    try:
        eng.check_error()
    except _lib.DLError as e:
        raised.append(str(e))
    assert len(raised) == 1 and "weight" in raised[0] and "global_step 3" in raised[0], raised
    for i, b in enumerate(bs[:3] + bs[4:]):
        twin.train_step(b, graph=i >= 1)
    torch.cuda.synchronize()
    twin.check_error()
    _same(eng, twin)
    assert int(eng.opt[7].item()) == int(twin.opt[7].item()) == 5


# --------------------------------------------------------------------------- 7. prefetch
def test_prefetched_weights_are_double_buffered(hip_lib):
    """train_step(batch, next_batch=...) with another weight vector in every batch equals the
    unprefetched run bit for bit: the next batch's weights, effective weights and normaliser land
    in the other buffer set while this step reads its own."""
    name, B = "deepfm_pipeline", 300
    bs = _batches(name, B, 4)
    bs[2] = dict(bs[2], weight=np.where(np.arange(B) % 3 == 0, 0, 2).astype(np.float32).reshape(B, 1))   # another N_nz
    mk = lambda: CTREngine(ModelSpec(name, pos_weight=PW, **KW[name]), max_batch=B, seed=6, adam="lazy",
                           sample_weight=True)
    a, b = mk(), mk()
    za, la = _run(a, bs, graph=True)
    zb, lb = _run(b, bs, graph=True, prefetch=True)
    for x, y in zip(za, zb):
        np.testing.assert_array_equal(x, y)
    assert la == lb
    _same(a, b)
    assert len(b._slots) >= 2 and b._slots[0]["w_eff"] is not b._slots[1]["w_eff"]
    assert b._slots[0]["norm"] is not b._slots[1]["norm"] and b._slots[0]["in_weight"] is not b._slots[1]["in_weight"]


# --------------------------------------------------------------------------- 8. eval stats
@pytest.mark.parametrize("n", [1, 67, 5000])
def test_eval_stats_weighted(hip_lib, n):
    """eval_stats(weights=) against numpy double at 1e-12 (relative), host and strided device
    inputs; all-ones weights give the unweighted values; a zero total weight gives NaN; a negative
    weight is refused."""
    rng = np.random.default_rng(n)
    s = rng.random(n).astype(np.float32)
    y = (rng.random(n) < 0.3).astype(np.float32)
    if n > 1:
        y[:2] = [1, 0]
    else:
        y[:] = 1
    w = _weights(n, 3) * (1 + rng.random(n).astype(np.float32))
    if not w.any():
        w[0] = 1
    want = W.eval_stats(y, s, w)
    pack = torch.from_numpy(np.stack([s, y, w], 1)).cuda()
    for got in (metrics.eval_stats(y, s, weights=w), metrics.eval_stats(pack[:, 1], pack[:, 0], weights=pack[:, 2])):
        for k in ("logloss", "calibration", "mean_score", "positive_rate", "weight_sum"):
            assert abs(got[k] - want[k]) <= 1e-12 * abs(want[k]), (k, got[k], want[k])
        assert got["n"] == n and got["n_nonzero"] == want["n_nonzero"]
    plain, ones = metrics.eval_stats(y, s), metrics.eval_stats(y, s, weights=np.ones(n, np.float32))
    for k in plain:
        assert abs(ones[k] - plain[k]) <= 1e-12 * abs(plain[k]), k
    z = metrics.eval_stats(y, s, weights=np.zeros(n, np.float32))
    assert np.isnan(z["logloss"]) and np.isnan(z["calibration"]) and z["weight_sum"] == 0 and z["n_nonzero"] == 0
    w[0] = -1
    with pytest.raises(ValueError, match="weights"):
        metrics.eval_stats(y, s, weights=w)
    acc = metrics.EvalAccumulator()
    acc.add(y, s, weights=np.ones(n, np.float32))
    with pytest.raises(ValueError, match="every batch"):
        acc.add(y, s)
        acc.add(y, s)


def test_ctr_model_eval_reports_weighted_stats(hip_lib):
    """CTRModel.eval on batches that carry a weight (weight_key=): logloss and calibration are the
    weighted ones of its scores, the AUC the same bits as without the weights."""
    from deep_learning_amd.models.deepfm_pipeline import DeepModel
    kw = KW["deepfm_pipeline"]
    args = types.SimpleNamespace(epochs=1, batch_size=67, model_pb="", save_model_checkpoint="", model_restore=0,
                                 restore_model_checkpoint="", embedding_size=kw["E"],
                                 cate_feats_size=kw["cate_index_size"], hidden_units=kw["hidden"], learning_rate=1e-3,
                                 l2_reg=1e-5, learning_rate_decay_steps=1000, learning_rate_decay_rate=0.9,
                                 cate_field_size=kw["S"], cont_field_size=kw["C"], vector_feats_size=0,
                                 eval_metrics=["auc", "logloss", "calibration"], weight_key="w", pos_weight=PW)
    bs = _batches("deepfm_pipeline", 67, 3)
    m = DeepModel(args, bs)
    assert m.spec.pos_weight == PW
    val = m.get_val_data(None, bs)
    assert len(val) == 5
    auc = m.eval(None, val)
    assert m.engine.weighted
    scores = np.concatenate([m.engine.predict({k: v for k, v in b.items() if k != "weight"}) for b in bs])
    y = np.concatenate([b["label"].reshape(-1) for b in bs])
    w = np.concatenate([b["weight"].reshape(-1) for b in bs])
    want = W.eval_stats(y, scores, w)
    for k in ("logloss", "calibration"):
        assert abs(m.last_eval[k] - want[k]) <= 1e-12 * abs(want[k]), k
    assert abs(want["logloss"] - metrics.eval_stats(y, scores)["logloss"]) > 1e-6
    args.weight_key = None
    m2 = DeepModel(args, bs)
    m2.engine = m.engine
    assert m2.eval(None, m2.get_val_data(None, [{k: v for k, v in b.items() if k != "weight"} for b in bs])) == auc
    assert auc == metrics.roc_auc(y, scores)
