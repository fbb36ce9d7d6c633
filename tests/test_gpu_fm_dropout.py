"""GPU checks of the FM part's dropout (include/dlamd.h "Dropout", dropout_keep_fm):
dl_head_fwd_bwd_fmdrop bit for bit against dl_head_fwd_bwd on numpy-masked features and the
numpy masks (tests/_fm_dropout_ref.py); the engine's logits, loss and embedding gradients
against the float64 autograd restatement fed the same masks, for every backward form; bit-exact
identities (lazy / dense, graph replay, all ones, predict); the sharded refusal.

Shapes.  A: deepfm_pipeline C = 13, S = 50, E = 8, B = 300: F = 63 (a ragged last Philox group),
fm_cols = 71 (the second-order columns straddle the two ballot words: 63 | 64..70), B no multiple
of the head's four-sample rounds.  B: the C2 field layout, C = 13, S = 26, E = 16: one ballot
word, four lanes per row.  C: deepfm_multi_cate with two pooled slots."""
import types

import numpy as np
import pytest
import torch

from deep_learning_amd import _lib
from deep_learning_amd._lib import call, ptr
from deep_learning_amd.engine import CTREngine, ModelSpec
from deep_learning_amd.synthetic import make_batch
from oracle import ctr_ref as R
from tests import _dropout_ref as D
from tests import _fm_dropout_ref as FD

pytestmark = pytest.mark.gpu

KEEPS = (0.7, 0.6)
B_ = 300
KWA = dict(C=13, S=50, E=8, cate_index_size=5000, hidden=[40, 24])
KWC = dict(V=4, S=8, E=16, cate_index_size=6000, hidden=[48, 32], multi_ranges=[[0, 30, "a"], [30, 50, "b"]])
SEED = 2019 + (7 << 32)      # both halves of the key in use


def _s():
    return _lib.stream_handle()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


# ------------------------------------------------------------------------------- head kernel
def _head_inputs(F, E, H, B=B_):
    g = torch.Generator().manual_seed(23)
    fm_cols = F + E
    fm_ld, ldh = (fm_cols + 3) // 4 * 4 + 4, H + 4
    fm = torch.randn(B, fm_ld, generator=g)
    h = torch.relu(torch.randn(B, ldh, generator=g))
    w = torch.randn(fm_cols + H + 1, generator=g) * 0.1
    y = (torch.rand(B, generator=g) < 0.3).float()
    return dict(F=F, E=E, H=H, B=B, fm_cols=fm_cols, fm_ld=fm_ld, ldh=ldh, fm=fm, h=h.cuda(), w=w.cuda(), y=y.cuda())


def _run_head(x, fm, drop=None, step=5):
    B, H, fm_cols = x["B"], x["H"], x["fm_cols"]
    grid = _lib.lib().dl_head_grid(B)
    out = dict(score=torch.zeros(B), z=torch.zeros(B), dz=torch.zeros(B), dh=torch.zeros(B, x["ldh"]),
               slab=torch.zeros(grid, fm_cols + H + 2))
    out = {k: v.cuda() for k, v in out.items()}
    fm = fm.cuda()
    args = [B, fm_cols, H, ptr(fm), x["fm_ld"], ptr(x["h"]), x["ldh"], ptr(x["w"]), ptr(x["y"]), 1e-7, 1.0 / B,
            ptr(out["score"]), ptr(out["z"]), ptr(out["dz"]), ptr(out["dh"]), ptr(out["slab"]), grid]
    if drop is None:
        call("dl_head_fwd_bwd", *args, _s())
    else:
        keeps, seed = drop
        opt = torch.zeros(_lib.OPT_LEN)
        opt[7] = step
        opt = opt.cuda()
        keep = torch.full((B, 2), -1, dtype=torch.int64, device="cuda")
        call("dl_head_fwd_bwd_fmdrop", *args, x["F"], D.keep_thr(keeps[0]), float(D.inv_keep(keeps[0])),
             D.keep_thr(keeps[1]), float(D.inv_keep(keeps[1])), seed, ptr(opt), ptr(keep), _s())
        out["keep"] = keep
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("F,E", [(63, 8), (39, 16)], ids=["A", "B"])
def test_head_twin_matches_masked_plain_head(hip_lib, F, E):
    """fm_keep is the numpy mask bit for bit (zeros past fm_cols); z, score, dz, dh and the slab
    equal dl_head_fwd_bwd's on a copy of fm_out masked and scaled in numpy float32, bit for bit;
    another step, seed or keep gives another mask; keeps (1, 0.6) keep every first-order column."""
    x = _head_inputs(F, E, 24)
    got = _run_head(x, x["fm"], (KEEPS, SEED))
    m1, m2 = FD.fm_masks(SEED, 5, B_, F, E, KEEPS)
    want_bits = FD.pack_keep(m1, m2)
    np.testing.assert_array_equal(got["keep"].view(np.uint64), want_bits)
    assert 0.6 < m1.mean() < 0.8 and 0.5 < m2.mean() < 0.7
    fm = x["fm"].numpy().copy()
    scale = np.concatenate([np.where(m1, D.inv_keep(KEEPS[0]), np.float32(0)),
                            np.where(m2, D.inv_keep(KEEPS[1]), np.float32(0))], 1).astype(np.float32)
    fm[:, :F + E] = fm[:, :F + E] * scale
    ref = _run_head(x, torch.from_numpy(fm))
    for k in ("z", "score", "dz", "dh", "slab"):
        assert np.array_equal(_bits(got[k]), _bits(ref[k])), k
    plain = _run_head(x, x["fm"])
    assert not np.array_equal(plain["z"], got["z"])
    for other in (dict(step=6), dict(drop=(KEEPS, SEED + 1)), dict(drop=((0.7, 0.5), SEED))):
        o = _run_head(x, x["fm"], other.get("drop", (KEEPS, SEED)), step=other.get("step", 5))
        assert not np.array_equal(o["keep"], got["keep"])
    one = _run_head(x, x["fm"], ((1.0, 0.6), SEED))
    first = FD.pack_keep(np.ones((B_, F), bool), FD.fm_masks(SEED, 5, B_, F, E, (1.0, 0.6))[1])
    np.testing.assert_array_equal(one["keep"].view(np.uint64), first)


# ------------------------------------------------------------------------------- engine
def _batch_a(seed, B=B_, kw=KWA):
    b = make_batch(B, cont=kw["C"], cate_fields=kw["S"], cate_index_size=kw["cate_index_size"], seed=seed)
    b["cate_feats"][0, :2] = [0, 1]      # the zero row, an id next to it
    return b


def _batch_c(seed, B, unique=False):
    """Shape C's batch.  unique: every multi-hot id appears once in the batch, in a range of its
    own — the dense engine adds the pooled gradients with atomics, whose order varies with two or
    more references to a row (tests/test_gpu_parity.py leaves the multi-hot models out of its
    lazy / dense identity for that reason); with one reference a row the sums have one order."""
    n1 = 2000 if unique else KWC["cate_index_size"]
    b = make_batch(B, cont=0, vector=KWC["V"], cate_fields=KWC["S"], cate_index_size=n1, seed=seed, cate_only=True)
    rng = np.random.default_rng(seed + 100)
    if unique:
        multi = n1 + rng.permutation(KWC["cate_index_size"] - n1)[:B * 50].reshape(B, 50)
    else:
        multi = rng.integers(1, KWC["cate_index_size"], size=(B, 50))
    multi[rng.random((B, 50)) < 0.5] = 0
    multi[0, :30] = 0                    # an empty slot: div_no_nan
    b["cate_feats"] = np.concatenate([b["cate_feats"], multi], 1)
    return b


def _params(cfg, seed=42):
    """The oracle's initial parameters: at B = 300 their FM gradients are large enough for the
    1e-5 bar to see a missing 1 / keep factor (asserted in parity_refs; on the CPU, float64:
    shape A 2.2e-2 first order, 1.8e-3 table; shape C 7.9e-4, 5.3e-5)."""
    return R.init_params(cfg, np.random.default_rng(seed))


@pytest.fixture(scope="module")
def parity_refs():
    """The float64 restatement's step on the masks of step 1 under seed 77, once per shape."""
    out = {}
    for name, model, kw, b in (("A", "deepfm_pipeline", KWA, _batch_a(11)),
                               ("C", "deepfm_multi_cate", KWC, _batch_c(11, B_))):
        cfg = R.make_cfg(model, **kw)
        P = _params(cfg)
        F, E = R.fm_fields(cfg), cfg.E
        m1, m2 = FD.fm_masks(77, 1, B_, F, E, KEEPS)
        inv = [D.inv_keep(k) for k in KEEPS]
        ref = FD.deepfm_fp64(cfg, P, b, m1, m2, *inv)
        # the 1e-5 bar must see a missing factor: the first-order gradient is all FM, so it times
        # (1 - keep) is what a missing 1 / keep loses; for the table, whose gradient also has the
        # tower's part, the restatement with the factors left out
        bare = FD.deepfm_fp64(cfg, P, b, m1, m2, 1.0, 1.0)
        assert np.abs(ref["G"]["fm_first_order_emb"] * (1 - KEEPS[0])).max() > 2e-5
        assert np.abs(ref["G"]["feats_emb"] - bare["G"]["feats_emb"]).max() > 2e-5
        out[name] = (model, kw, cfg, P, b, (m1, m2), ref)
    return out


def _engine(model, kw, P=None, keeps=KEEPS, seed=77, B=B_, **ekw):
    spec = ModelSpec(model, dropout_keep_fm=keeps, **kw)
    eng = CTREngine(spec, max_batch=B, seed=seed, **({"init": "none"} if P is not None else {}), **ekw)
    if P is not None:
        eng.load_params({k: v.copy() for k, v in P.items()})
    return eng


def _step_with_grads(eng, b):
    """One eager train_step; the table / first-order gradient buffers and dx0 as the embedding
    backward left them (copied when the head's Adam, the launch after it, is issued: the row
    Adams zero the buffers)."""
    snap = {}
    orig = eng._c

    def spy(label, name, *a):
        if label == "adam_head" and eng.tg is not None:
            snap["tg"], snap["fmg"] = eng.tg.clone(), eng.fmg.clone()
        return orig(label, name, *a)
    eng._c = spy
    eng.train_step(b)
    torch.cuda.synchronize()
    eng.check_error()
    eng._c = orig
    return {k: v.cpu().numpy() for k, v in snap.items()}


@pytest.mark.parametrize("shape,mode", [("A", "sorted"), ("A", "atomic"), ("A", "lazy"), ("C", "sorted")])
def test_engine_gradients_match_fp64(hip_lib, parity_refs, shape, mode):
    """One train_step from loaded parameters: logits and loss, and for the dense forms the table
    and first-order gradients and dx0, within the project's 1e-5 of the float64 restatement fed
    the numpy masks.  Measured max |engine - fp64| is printed."""
    model, kw, cfg, P, b, (m1, m2), ref = parity_refs[shape]
    ekw = {"adam": "lazy"} if mode == "lazy" else {"bwd": mode}
    eng = _engine(model, kw, P, **ekw)
    g = _step_with_grads(eng, b)
    assert int(eng.opt[7].item()) == 1
    np.testing.assert_array_equal(eng.fm_keep[:B_].cpu().numpy().view(np.uint64), FD.pack_keep(m1, m2))
    err = {"z": np.abs(eng.z[:B_].cpu().numpy() - ref["z"]).max(), "loss": abs(eng.loss() - ref["loss"])}
    if mode != "lazy":
        N, S, E, M = eng.N, cfg.S, cfg.E, ref["M"]
        err["table"] = np.abs(g["tg"][:N] - ref["G"]["feats_emb"]).max()
        err["first"] = np.abs(g["fmg"][:N] - ref["G"]["fm_first_order_emb"][:, 0]).max()
        dx0 = eng.dx0[:B_, :(S + M) * E].cpu().numpy()          # internal columns [single cate | pooled]
        c0 = cfg.C + cfg.V                                       # reference columns [cont, vector, single, pooled]
        err["dx0"] = np.abs(dx0 - ref["dx0"][:, c0:c0 + (S + M) * E]).max()
    print("max |engine - fp64|:", {k: float(v) for k, v in err.items()})
    for k, v in err.items():
        assert v < 1e-5, (k, v)


def _train(eng, bs, graph):
    zs = []
    for b in bs:
        eng.train_step(b, graph=graph)
        torch.cuda.synchronize()
        zs.append(eng.z[: eng.last_batch].cpu().numpy().copy())
    eng.check_error()
    return zs


def _same_params(a, b):
    pa, pb = a.params(), b.params()
    for k in pa:
        np.testing.assert_array_equal(pa[k], pb[k], err_msg=k)


@pytest.mark.parametrize("shape", ["A", "C"])
def test_lazy_equals_dense_sorted(hip_lib, shape):
    """Lazy records against the dense sorted backward, both dropping: logits of 3 steps and the
    parameters bit for bit."""
    if shape == "A":
        model, kw, B = "deepfm_pipeline", KWA, B_
        bs = [_batch_a(60 + i) for i in range(3)]
    else:
        model, kw, B = "deepfm_multi_cate", KWC, 64
        bs = [_batch_c(60 + i, B, unique=True) for i in range(3)]
    dense = _engine(model, kw, seed=3, B=B, bwd="sorted")
    lazy = _engine(model, kw, seed=3, B=B, adam="lazy")
    zd, zl = _train(dense, bs, graph=False), _train(lazy, bs, graph=False)
    for a, b in zip(zd, zl):
        np.testing.assert_array_equal(a, b)
    _same_params(dense, lazy)
    plain = CTREngine(ModelSpec(model, **kw), max_batch=B, seed=3, bwd="sorted")
    assert not np.array_equal(_train(plain, bs[:1], graph=False)[0], zd[0])      # and it is not the undropped model


def test_graph_replay_equals_eager_and_the_mask_advances(hip_lib):
    """Shape A, lazy Adam: 3 graph steps equal 3 eager steps of another engine with the same seed
    bit for bit; the same batch repeated sees step 1's and then step 2's mask (fm_keep is a static
    buffer the replayed head rewrites from opt[7])."""
    b = _batch_a(31)
    bs = [b, b, _batch_a(32)]
    eager, graph = (_engine("deepfm_pipeline", KWA, seed=9, adam="lazy") for _ in range(2))
    F, E = 63, 8
    keeps = []
    for i, bb in enumerate(bs):
        eager.train_step(bb)
        graph.train_step(bb, graph=True)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(graph.z[:B_].cpu().numpy(), eager.z[:B_].cpu().numpy(), err_msg="step %d" % i)
        keeps.append(graph.fm_keep[:B_].cpu().numpy().view(np.uint64).copy())
        np.testing.assert_array_equal(keeps[-1], FD.pack_keep(*FD.fm_masks(9, i + 1, B_, F, E, KEEPS)))
    graph.check_error()
    _same_params(eager, graph)
    assert not np.array_equal(keeps[0], keeps[1])


def _labels(eng, b):
    eng.prof = []
    eng.train_step(b)
    torch.cuda.synchronize()
    out = [p[0] for p in eng.prof]
    eng.prof = None
    return out


@pytest.mark.parametrize("adam", ["lazy", "dense"])
def test_all_ones_is_the_engine_without_dropout(hip_lib, adam):
    """All-ones keeps: 3 steps bit-identical to an engine built without the argument, the same
    launch labels — which an engine that does drop keeps too."""
    bs = [_batch_a(20 + i) for i in range(4)]
    ekw = {"adam": "lazy"} if adam == "lazy" else {"bwd": "sorted"}
    engs = [CTREngine(ModelSpec("deepfm_pipeline", **KWA, **kw), max_batch=B_, seed=5, **ekw)
            for kw in ({}, {"dropout_keep_fm": [1, 1]})]
    assert engs[1].fmdrop is None and not hasattr(engs[1], "fm_keep")
    za, zb = (_train(e, bs[:3], graph=False) for e in engs)
    for a, b in zip(za, zb):
        np.testing.assert_array_equal(a, b)
    _same_params(*engs)
    la, lb = (_labels(e, bs[3]) for e in engs)
    assert la == lb
    drop = _engine("deepfm_pipeline", KWA, seed=5, **ekw)
    assert _labels(drop, bs[3]) == la
    assert {"head", "embed_bwd", "cont_bwd"} <= set(la)


def test_predict_never_drops(hip_lib):
    cfg = R.make_cfg("deepfm_pipeline", **KWA)
    P = _params(cfg)
    b = _batch_a(41)
    out = []
    for keeps in (None, KEEPS):
        eng = _engine("deepfm_pipeline", KWA, P, keeps=keeps, seed=3)
        out.append(eng.predict(b, logits=True))
    np.testing.assert_array_equal(out[0], out[1])


def test_with_deep_dropout_together(hip_lib):
    """dropout_keep_fm and dropout_keep_deep together train, lazy equal to dense, and differ from
    either alone."""
    bs = [_batch_a(70 + i) for i in range(2)]
    deep = (1, 0.8, 0.7)
    z = {}
    for name, kw in (("fm", dict(dropout_keep_fm=KEEPS)), ("deep", dict(dropout_keep_deep=deep)),
                     ("both", dict(dropout_keep_fm=KEEPS, dropout_keep_deep=deep))):
        eng = CTREngine(ModelSpec("deepfm_pipeline", **KWA, **kw), max_batch=B_, seed=4, adam="lazy")
        z[name] = _train(eng, bs, graph=True)
        assert np.isfinite(z[name][1]).all()
        if name == "both":
            dense = CTREngine(ModelSpec("deepfm_pipeline", **KWA, **kw), max_batch=B_, seed=4, bwd="sorted")
            for a, b in zip(_train(dense, bs, graph=False), z[name]):
                np.testing.assert_array_equal(a, b)
            _same_params(dense, eng)
    assert not np.array_equal(z["both"][0], z["fm"][0]) and not np.array_equal(z["both"][0], z["deep"][0])


def test_sharded_engine_refuses(hip_lib):
    from deep_learning_amd.shard import ShardedCTREngine
    pk = dict(C=13, S=26, E=8, cate_index_size=3000, hidden=[40, 24])
    with pytest.raises(ValueError, match="dropout_keep_fm"):
        ShardedCTREngine(ModelSpec("deepfm_pipeline", dropout_keep_fm=KEEPS, **pk), 64,
                         types.SimpleNamespace(world=1, rank=0))
