"""GPU checks of the deep tower's dropout (include/dlamd.h "Dropout"): dl_dropout_apply and
dl_gemm_s3_nt_drop bit for bit against their undropped twins and the numpy mask
(tests/_dropout_ref.py); the engine's logits, loss and stage gradients against the float64
autograd restatement fed the same masks; identities (no dropout, graph replay, seed,
predict, lazy / dense) bit-exact; the refused combinations.

Kernel shapes: the s3 NT tile is 256 rows x 208 columns, so M = 300, N = 230 gives two row
tiles (the second ragged), a second column tile and N % 16 != 0 (the epilogue through LDS);
N = 232 with ldc % 4 == 0 takes the register epilogue."""
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

pytestmark = pytest.mark.gpu

M_, K_ = 300, 96
SEED = 2019 + (7 << 32)      # both halves of the key in use
STEP, LAYER, KEEP = 5, 2, 0.8
SHAPES = [(230, 233), (232, 236)]      # (N, ldc): the LDS epilogue, the register epilogue


def _s():
    return _lib.stream_handle()


def _opt(step=STEP):
    o = torch.zeros(_lib.OPT_LEN)
    o[7] = step
    return o.cuda()


def _drop(keep=KEEP, seed=SEED, layer=LAYER):
    return D.keep_thr(keep), float(D.inv_keep(keep)), seed, layer


def _planes(W):
    rows, cols = W.shape
    P = torch.zeros(3 * rows * cols, dtype=torch.int16, device="cuda")
    call("dl_split3", ptr(W), rows, cols, cols, 0, ptr(P), cols, rows * cols, _s())
    return P


def _unpack(bits, N):
    """bool [M][16 ceil(N / 16)] of the halfwords' bits."""
    b = bits.cpu().numpy().view(np.uint16)[:, : (N + 15) // 16].astype(np.uint32)
    return ((b[:, :, None] >> np.arange(16, dtype=np.uint32)) & 1).astype(bool).reshape(b.shape[0], -1)


def _bits_eq(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.int32),
                          np.ascontiguousarray(b, np.float32).view(np.int32))


@pytest.fixture(scope="module")
def operands():
    g = torch.Generator().manual_seed(17)
    lda = K_ + 4
    A = torch.zeros(M_, lda)
    A[:, :K_] = torch.randn(M_, K_, generator=g)
    out = {"A": A.cuda(), "lda": lda}
    for N, _ in SHAPES:
        Bm = (torch.randn(N, K_, generator=g) * 0.05).cuda()
        out[N] = _planes(Bm)
    torch.cuda.synchronize()
    return out


@pytest.fixture(scope="module")
def mask_ref():
    return {N: D.keep_mask(SEED, STEP, LAYER, M_, N, KEEP) for N, _ in SHAPES}


@pytest.mark.parametrize("N,ld", SHAPES)
def test_dropout_apply_matches_numpy(hip_lib, mask_ref, N, ld):
    """mask_out equals the numpy mask bit for bit; in place, columns [0, N) become
    keep ? x * inv : 0 and the columns past N stay."""
    thr, inv, seed, layer = _drop()
    opt = _opt()
    mo = torch.full((M_, N), 9, dtype=torch.uint8, device="cuda")
    call("dl_dropout_apply", None, M_, N, 0, thr, inv, seed, layer, ptr(opt), ptr(mo), _s())
    g = torch.Generator().manual_seed(N)
    x0 = torch.randn(M_, ld, generator=g)
    x = x0.cuda()
    mo2 = torch.zeros(M_, N, dtype=torch.uint8, device="cuda")
    call("dl_dropout_apply", ptr(x), M_, N, ld, thr, inv, seed, layer, ptr(opt), ptr(mo2), _s())
    torch.cuda.synchronize()
    mask = mask_ref[N]
    assert np.array_equal(mo.cpu().numpy().astype(bool), mask) and int(mo.max()) == 1
    assert torch.equal(mo, mo2)
    want = x0.numpy().copy()
    want[:, :N] = np.where(mask, want[:, :N] * np.float32(inv), np.float32(0))
    assert _bits_eq(x.cpu().numpy(), want)
    # another step, layer or seed: another mask
    for kw in (dict(step=STEP + 1), dict(layer=LAYER + 1), dict(seed=SEED + 1)):
        o2 = _opt(kw.get("step", STEP))
        call("dl_dropout_apply", None, M_, N, 0, thr, inv, kw.get("seed", seed), kw.get("layer", layer), ptr(o2),
             ptr(mo2), _s())
        torch.cuda.synchronize()
        want2 = D.keep_mask(kw.get("seed", SEED), kw.get("step", STEP), kw.get("layer", LAYER), M_, N, KEEP)
        assert np.array_equal(mo2.cpu().numpy().astype(bool), want2) and not np.array_equal(want2, mask)


@pytest.mark.parametrize("N,ldc", SHAPES)
def test_gemm_drop_relu_epilogue(hip_lib, operands, mask_ref, N, ldc):
    """epi 1: C = where(mask, relu * inv, 0) of dl_gemm_s3_nt_bits' C bit for bit, the bitmask
    = its bitmask AND the mask, bits past N in the last halfword zero, halfwords and columns
    past the matrix untouched; bits = NULL writes the same C."""
    thr, inv, seed, layer = _drop()
    opt = _opt()
    A, lda, Bp = operands["A"], operands["lda"], operands[N]
    ldbits = 32
    C0 = torch.full((M_, ldc), 7.0, device="cuda")
    C1, C2 = C0.clone(), C0.clone()
    b0 = torch.full((M_, ldbits), -1, dtype=torch.int16, device="cuda")
    b1 = b0.clone()
    call("dl_gemm_s3_nt_bits", M_, N, K_, ptr(A), lda, ptr(Bp), K_, N * K_, ptr(C0), ldc, 1, None, 0, ptr(b0),
         ldbits, _s())
    call("dl_gemm_s3_nt_drop", M_, N, K_, ptr(A), lda, ptr(Bp), K_, N * K_, ptr(C1), ldc, 1, None, 0, ptr(b1),
         ldbits, thr, inv, seed, layer, ptr(opt), _s())
    call("dl_gemm_s3_nt_drop", M_, N, K_, ptr(A), lda, ptr(Bp), K_, N * K_, ptr(C2), ldc, 1, None, 0, None, 0,
         thr, inv, seed, layer, ptr(opt), _s())
    torch.cuda.synchronize()
    mask = mask_ref[N]
    c0 = C0.cpu().numpy()
    assert (c0[:, :N] > 0).mean() > 0.3          # the product is not trivially zero
    want = c0.copy()
    want[:, :N] = np.where(mask, c0[:, :N] * np.float32(inv), np.float32(0))
    assert _bits_eq(C1.cpu().numpy(), want)
    assert torch.equal(C1, C2)
    u0, u1 = _unpack(b0, N), _unpack(b1, N)
    assert np.array_equal(u0[:, :N], c0[:, :N] > 0)
    assert np.array_equal(u1[:, :N], u0[:, :N] & mask)
    assert not u1[:, N:].any()
    nh = (N + 15) // 16
    assert (b1[:, nh:] == -1).all()


@pytest.mark.parametrize("N,ldc", SHAPES)
def test_gemm_drop_bitmask_epilogue(hip_lib, operands, N, ldc):
    """epi 3 equals dl_gemm_s3_nt_bits' epi 3 times inv, bit for bit."""
    thr, inv, seed, layer = _drop()
    opt = _opt()
    A, lda, Bp = operands["A"], operands["lda"], operands[N]
    ldbits = 32
    g = torch.Generator().manual_seed(N + 1)
    bits = torch.randint(-32768, 32768, (M_, ldbits), generator=g, dtype=torch.int32).to(torch.int16).cuda()
    C0 = torch.full((M_, ldc), 7.0, device="cuda")
    C1 = C0.clone()
    call("dl_gemm_s3_nt_bits", M_, N, K_, ptr(A), lda, ptr(Bp), K_, N * K_, ptr(C0), ldc, 3, None, 0, ptr(bits),
         ldbits, _s())
    call("dl_gemm_s3_nt_drop", M_, N, K_, ptr(A), lda, ptr(Bp), K_, N * K_, ptr(C1), ldc, 3, None, 0, ptr(bits),
         ldbits, thr, inv, seed, layer, ptr(opt), _s())
    torch.cuda.synchronize()
    c0 = C0.cpu().numpy()
    assert 0.3 < (c0[:, :N] != 0).mean() < 0.7
    want = c0.copy()
    want[:, :N] = c0[:, :N] * np.float32(inv)
    assert _bits_eq(C1.cpu().numpy(), want)


def test_gemm_drop_refuses_other_epilogues(hip_lib, operands):
    N, ldc = SHAPES[1]
    C = torch.zeros(M_, ldc, device="cuda")
    thr, inv, seed, layer = _drop()
    for epi in (0, 2):
        with pytest.raises(_lib.DLError):
            call("dl_gemm_s3_nt_drop", M_, N, K_, ptr(operands["A"]), operands["lda"], ptr(operands[N]), K_, N * K_,
                 ptr(C), ldc, epi, ptr(C), ldc, None, 0, thr, inv, seed, layer, ptr(_opt()), _s())


# ------------------------------------------------------------------------------- engine
KW = dict(S=6, E=8, cate_index_size=2000, hidden=[230, 48, 24])
KEEPS = (0.9, 0.8, 0.8, 0.7)
B_ = 300


def _batch(seed, B=B_, **kw):
    b = make_batch(B, cont=0, cate_fields=KW["S"], cate_index_size=KW["cate_index_size"], seed=seed, cate_only=True,
                   **kw)
    b["cate_feats"][0, :2] = [0, 1]
    return b


@pytest.fixture(scope="module")
def parity_ref():
    """The float64 restatement's step on the masks of step 1 under seed 77, computed once."""
    cfg = R.make_cfg("dnn_cate", **KW)
    P = R.init_params(cfg, np.random.default_rng(42))
    b = _batch(11)
    dims = [KW["S"] * KW["E"]] + KW["hidden"]
    masks = [D.keep_mask(77, 1, l, B_, d, KEEPS[l]) for l, d in enumerate(dims)]
    ref = D.dnn_cate_fp64(cfg, P, b, masks, [D.inv_keep(k) for k in KEEPS])
    return cfg, P, b, masks, ref


@pytest.mark.parametrize("adam", ["dense", "lazy"])
def test_engine_gradients_match_fp64(hip_lib, parity_ref, adam):
    """One train_step from loaded parameters: logits, loss and the gradients themselves (every
    layer's dh and dx0) within the project's 1e-5 of the float64 restatement fed the numpy masks;
    a dropped element's activation and gradient are exactly zero."""
    cfg, P, b, masks, ref = parity_ref
    spec = ModelSpec("dnn_cate", dropout_keep_deep=KEEPS, **KW)
    eng = CTREngine(spec, max_batch=B_, init="none", adam=adam, seed=77,
                    **({} if adam == "lazy" else {"bwd": "sorted"}))
    eng.load_params({k: v.copy() for k, v in P.items()})
    eng.train_step(b)
    torch.cuda.synchronize()
    eng.check_error()
    assert int(eng.opt[7].item()) == 1
    z = eng.z[:B_].cpu().numpy()
    err = {"z": np.abs(z - ref["z"]).max(), "loss": abs(eng.loss() - ref["loss"])}
    hid = KW["hidden"]
    dx0 = eng.dx0[:B_, : KW["S"] * KW["E"]].cpu().numpy()
    err["dx0"] = np.abs(dx0 - ref["dx0"]).max()
    for l, h in enumerate(hid):
        dh = eng.dh[l][:B_, :h].cpu().numpy()
        err["dh%d" % l] = np.abs(dh - ref["dh"][l]).max()
        hl = eng.h[l][:B_, :h].cpu().numpy()
        assert np.all(hl[~masks[l + 1]] == 0) and np.all(dh[~masks[l + 1]] == 0)
        assert (hl[masks[l + 1]] > 0).mean() > 0.2
        assert np.all(eng.h[l][:B_, h].cpu().numpy() == 1)      # the bias "ones" column is not dropped
    assert np.all(dx0[~masks[0]] == 0)
    x0 = eng.x0[:B_, : KW["S"] * KW["E"]].cpu().numpy()
    assert np.all(x0[~masks[0]] == 0) and np.all(eng.x0[:B_, eng.D0].cpu().numpy() == 1)
    print("max |engine - fp64|:", {k: float(v) for k, v in err.items()},
          "max |ref dh|:", [float(np.abs(g).max()) for g in ref["dh"]])
    for k, v in err.items():
        assert v < 1e-5, (k, v)
    # the gradients are 1/B-sized: the 1e-5 bar must still see a missing 1/keep factor
    for l in range(len(hid)):
        assert np.abs(ref["dh"][l] * (1 - KEEPS[l + 1])).max() > 2e-5


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


def _labels(eng, b):
    eng.prof = []
    eng.train_step(b)
    torch.cuda.synchronize()
    out = [p[0] for p in eng.prof]
    eng.prof = None
    return out


def test_all_ones_is_the_engine_without_dropout(hip_lib):
    """An all-ones keep list: 3 steps bit-identical to an engine built without the argument, the
    same launches."""
    bs = [_batch(20 + i) for i in range(4)]
    engs = [CTREngine(ModelSpec("dnn_cate", **KW, **kw), max_batch=B_, seed=5, adam="lazy")
            for kw in ({}, {"dropout_keep_deep": [1, 1, 1, 1, 1]})]
    assert engs[1].drop is None and engs[1].fused_gather_rows() == engs[0].fused_gather_rows()
    za, zb = (_train(e, bs[:3], graph=False) for e in engs)
    for a, b in zip(za, zb):
        np.testing.assert_array_equal(a, b)
    _same_params(*engs)
    la, lb = (_labels(e, bs[3]) for e in engs)
    assert la == lb and not any(x.startswith("drop") for x in la)
    # and an engine that does drop launches the dropout passes
    eng = CTREngine(ModelSpec("dnn_cate", dropout_keep_deep=KEEPS, **KW), max_batch=B_, seed=5, adam="lazy")
    ld = _labels(eng, bs[3])
    assert [x for x in ld if x.startswith("drop")] == ["drop_x0", "drop_dh", "drop_dx0"]


def test_graph_replay_equals_eager_and_the_mask_advances(hip_lib):
    """deepfm_pipeline, lazy Adam, with dropout: 3 graph steps equal 3 eager steps of another
    engine with the same seed bit for bit (so two engines with one seed agree, and the replayed
    graph draws step t's mask from opt[7]); another seed trains differently; the same batch
    repeated sees step 1's and then step 2's mask."""
    kw = dict(C=13, S=26, E=8, cate_index_size=3000, hidden=[40, 24])
    keeps = (0.9, 0.8, 0.7)
    spec = ModelSpec("deepfm_pipeline", dropout_keep_deep=keeps, **kw)
    b = make_batch(B_, cate_index_size=kw["cate_index_size"], seed=31)
    bs = [b, b, make_batch(B_, cate_index_size=kw["cate_index_size"], seed=32)]
    eager = CTREngine(spec, max_batch=B_, seed=9, adam="lazy")
    graph = CTREngine(spec, max_batch=B_, seed=9, adam="lazy")
    other = CTREngine(spec, max_batch=B_, seed=9, adam="lazy")
    other.seed = 10       # the same initial parameters, another mask
    ze = []
    h0 = []
    losses = []
    for i, bb in enumerate(bs):
        eager.train_step(bb)
        graph.train_step(bb, graph=True)
        torch.cuda.synchronize()
        ze.append(eager.z[:B_].cpu().numpy().copy())
        np.testing.assert_array_equal(graph.z[:B_].cpu().numpy(), ze[-1], err_msg="step %d" % i)
        h0.append(graph.h[0][:B_, :40].cpu().numpy().copy())
        losses.append(graph.loss())
        assert int(graph.opt[7].item()) == i + 1
    _same_params(eager, graph)
    zo = _train(other, bs[:1], graph=False)
    assert not np.array_equal(zo[0], ze[0])
    # the repeated batch: each replay dropped its own step's mask
    assert losses[0] != losses[1]
    for step in (1, 2):
        m = D.keep_mask(9, step, 1, B_, 40, keeps[1])
        assert np.all(h0[step - 1][~m] == 0)
        assert (h0[2 - step][~m] != 0).any()


def test_predict_never_drops(hip_lib):
    cfg = R.make_cfg("dnn_cate", **KW)
    P = R.init_params(cfg, np.random.default_rng(42))
    b = _batch(41)
    out = []
    for kw in ({}, {"dropout_keep_deep": KEEPS}):
        eng = CTREngine(ModelSpec("dnn_cate", **KW, **kw), max_batch=B_, init="none", seed=3)
        eng.load_params({k: v.copy() for k, v in P.items()})
        out.append(eng.predict(b, logits=True))
    np.testing.assert_array_equal(out[0], out[1])
    np.testing.assert_allclose(out[1], R.forward(cfg, P, b)["z"], atol=1e-5, rtol=0)


def test_wdl_lazy_wide_equals_dense_with_dropout(hip_lib):
    """wdl, f32 tower: lazy tables + lazy wide records on graph steps against the eager dense-Adam
    engine, both dropping: logits of 3 steps and the parameters bit for bit (the wide rows that
    alias h[-1] see the dropped activations on both)."""
    kw = dict(C=13, S=26, E=16, cate_index_size=8000, hidden=[64, 32], Fw=26)
    spec = ModelSpec("wdl", dropout_keep_deep=(0.9, 0.8, 0.7), **kw)
    bs = [make_batch(128, cate_index_size=kw["cate_index_size"], seed=50 + i, wide_fields=26) for i in range(3)]
    Fw, H = kw["Fw"], kw["hidden"][-1]
    for j, b in enumerate(bs):
        b["wide_feats"][j, :3] = [Fw + j, Fw + H - 1, Fw]      # wide ids on the deep-output rows
    dense = CTREngine(spec, max_batch=128, seed=3, bwd="sorted")
    lazy = CTREngine(spec, max_batch=128, seed=3, adam="lazy")
    assert lazy.wide_lazy and lazy.drop and not lazy.fused_gather_rows()
    zd, zl = _train(dense, bs, graph=False), _train(lazy, bs, graph=True)
    for a, b in zip(zd, zl):
        np.testing.assert_array_equal(a, b)
    _same_params(dense, lazy)
    # and it is not the undropped model
    plain = CTREngine(ModelSpec("wdl", **kw), max_batch=128, seed=3, bwd="sorted")
    assert not np.array_equal(_train(plain, bs[:1], graph=False)[0], zd[0])


def test_refused_combinations(hip_lib):
    keeps = {"dropout_keep_deep": KEEPS}
    with pytest.raises(ValueError, match="bf16"):
        CTREngine(ModelSpec("dnn_cate", tower="bf16", **KW, **keeps), max_batch=64)
    with pytest.raises(ValueError, match="gemm='f32'"):
        CTREngine(ModelSpec("dnn_cate", **KW, **keeps), max_batch=64, gemm="f32")
    from deep_learning_amd.shard import ShardedCTREngine
    pk = dict(C=13, S=26, E=8, cate_index_size=3000, hidden=[40, 24])
    with pytest.raises(ValueError, match="ShardedCTREngine"):
        ShardedCTREngine(ModelSpec("dnn_pipeline", dropout_keep_deep=(1, 0.8, 0.8), **pk), 64,
                         types.SimpleNamespace(world=1, rank=0))
    mk = dict(V=4, S=8, E=16, cate_index_size=6000, hidden=[48, 32], multi_ranges=[[0, 30, "a"], [30, 50, "b"]])
    with pytest.raises(ValueError, match="multi-hot"):
        CTREngine(ModelSpec("deepfm_multi_cate", dropout_keep_deep=(0.9, 0.8, 0.8), **mk), max_batch=64)
    # no dropout: every one of them still builds
    CTREngine(ModelSpec("dnn_cate", dropout_keep_deep=[1, 1, 1, 1], **KW), max_batch=64)
