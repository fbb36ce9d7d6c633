"""The lookup, record and pooling kernels at the edges of what ModelSpec accepts (tests/_envelope.py): the
embedding sizes 4, 32 and 64, the forward's slot-count arms up to its 128-slot limit, 16 / 17 / 32 FM cont
fields, batches around the 16-sample tile and past the backward's and the forward's grids, and rows that
return after lagging past the catch-up's 256-step window.

Every training case is checked three ways: the trajectory against the float32 oracle at TOL; the forward's
outputs for copies and single products bit for bit; and the first step's gradient itself, recovered from
the exported first moments as m / (1 - beta1), against the oracle's float64 backward within REL of each
array's largest value, with every untouched table row exactly 0.  The last is the check with room to spare:
Adam's step moves little when a gradient is scaled, so a row added twice shows in the trajectory by a small
margin or not at all, and in the gradient by orders of magnitude (profiles/envelope/README.md: two such
mutations of the E = 64 atomic backward, tried on deepfm_pipeline-E64-C13-V0-S26-B300-atomic).

Measured maxima are printed one ENVELOPE_ERR line a case (profiles/envelope/errors.txt)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from deep_learning_amd import _lib  # noqa: E402
from deep_learning_amd.engine import CTREngine, ModelSpec  # noqa: E402
from oracle import ctr_ref as R  # noqa: E402
from tests import _envelope as V  # noqa: E402

TOL, REL = V.TOL, V.REL
_RUNS = {}


def _engine(spec, B, mode, **kw):
    if mode == "lazy":
        return CTREngine(spec, max_batch=B, init="none", adam="lazy", **kw)
    return CTREngine(spec, max_batch=B, init="none", bwd=mode, **kw)


def _gradients(eng, ref):
    """The gradient the engine applied at its first step, per reference parameter: m / (1 - beta1).
    (adam_state() flushes a lazy table: the lazy cases' remaining steps start from caught-up records, so
    their rows lag two steps at most.  The sizes are what these cases are about; lag is
    test_catch_up_past_the_window_bit_identical_to_dense's, and at E = 8 / 16 test_gpu_parity.py's.)"""
    sp = eng.spec
    st, ds = eng.adam_state(), eng.dense_state()["m"]
    m = {sp.table_key: st["m"].reshape(ref["P0"][sp.table_key].shape)}
    if sp.fm:
        m[sp.first_key] = st["m1"].reshape(ref["P0"][sp.first_key].shape)
    for k in ref["P0"]:
        if k not in m:
            m[k] = ds[k].reshape(ref["P0"][k].shape)
    return {k: v.astype(np.float64) / V.ONE_MINUS_BETA1 for k, v in m.items()}


def _check_forward(eng, ref, B):
    """x0 and fm_out after the first step's forward against the float32 oracle's: copies and single
    products exact, sums at the tolerances of test_embed_fwd_bit_exact_gather / test_pool_counts_bit_exact."""
    sp, fw = eng.spec, ref["fw0"]
    S, E, M, C, Vv = sp.S, sp.E, sp.M, sp.C, sp.V
    x0 = eng.x0[:B].cpu().numpy()
    same = np.testing.assert_array_equal
    same(x0[:, :S * E], fw["x0"][:, C + Vv: C + Vv + S * E], err_msg="x0 single-valued columns")
    same(x0[:, eng.cont_col: eng.cont_col + C], fw["x0"][:, :C], err_msg="x0 cont columns")
    same(x0[:, eng.vec_col: eng.vec_col + Vv], fw["x0"][:, C: C + Vv], err_msg="x0 vector columns")
    if M:
        np.testing.assert_allclose(x0[:, S * E: (S + M) * E], fw["x0"][:, C + Vv + S * E:], rtol=1e-6, atol=1e-7)
    if sp.fm:
        fo = eng.fm_out[:B].cpu().numpy()
        n1 = sp.F - M
        same(fo[:, :n1], fw["first"][:, :n1], err_msg="first-order columns")
        if M:
            np.testing.assert_allclose(fo[:, n1: sp.F], fw["first"][:, n1:], rtol=1e-6, atol=1e-7)
        np.testing.assert_allclose(fo[:, sp.F: sp.F + E], fw["second"], rtol=1e-5, atol=1e-6)


def _run(c):
    """One case, run once: every check against the oracle, the measured maxima printed; returns what the
    bit-identity tests compare (logits of every step, final parameters, the first step's moments)."""
    cid = V.case_id(c)
    if cid in _RUNS:
        return _RUNS[cid]
    model, kw, B, mode = c
    ref = V.case_reference(c)
    spec = ModelSpec(model, **kw)
    eng = _engine(spec, B, mode)
    eng.load_params(ref["P0"])
    grads = c in V.GRADIENT_CASES
    zs, ez, el, gerr, m1 = [], 0.0, 0.0, {}, None
    for step, b in enumerate(ref["batches"]):
        eng.train_step(b, graph=(step >= 2))
        torch.cuda.synchronize()
        eng.check_error()
        z = eng.z[:B].cpu().numpy().copy()
        zs.append(z)
        ez = max(ez, float(np.abs(z - ref["zs"][step]).max()))
        el = max(el, abs(eng.loss() - ref["losses"][step]))
        if step == 0:
            _check_forward(eng, ref, B)
            if grads:
                G = _gradients(eng, ref)
                gerr = V.grad_errors(G, ref["G64"])
                m1 = G
    got = eng.params()
    ep = max(float(np.abs(got[k] - ref["P"][k]).max()) for k in ref["P"])
    print("ENVELOPE_ERR %s z=%.3g loss=%.3g params=%.3g grad=%.3g (%s)"
          % (cid, ez, el, ep, max(gerr.values()) if gerr else float("nan"),
             max(gerr, key=gerr.get) if gerr else "no gradient check"))
    assert ez <= TOL and el < TOL and ep <= TOL, (ez, el, ep)
    if grads:
        for k, e in gerr.items():
            assert e < REL, (k, e)
        # rows no reference touched: exactly 0 (a stray add would hide below REL of the largest row)
        for k in (spec.table_key,) + ((spec.first_key,) if spec.fm else ()):
            g64 = ref["G64"][k]
            idle = np.abs(g64).reshape(g64.shape[0], -1).max(1) == 0
            assert idle.any() and not np.asarray(m1[k]).reshape(g64.shape)[idle].any(), k
        if spec.model == "wdl":
            # the wide rows no sample names (lazy: records the step never touched, replayed by the flush):
            # the L2 term l2 * w alone.  Not 0, so not exact: float32(l2) is within half an ulp of l2, the
            # product, the moment's factor and its recovery round once each: 4 ulp of l2 * w covers them
            w = ref["P0"]["wdl_weights"].astype(np.float64)
            g64 = ref["G64"]["wdl_weights"]
            idle = g64 == ref["cfg"].l2 * w
            rel = np.abs(m1["wdl_weights"][idle] - g64[idle]) / np.abs(g64[idle])
            print("ENVELOPE_ERR %s wide rows untouched: %d, worst %.3g ulp of l2 * w"
                  % (cid, idle.sum(), float(rel.max()) * 2.0 ** 24))
            assert idle.any() and rel.max() <= 4 * 2.0 ** -24
    _RUNS[cid] = dict(zs=zs, params=got, grads=m1)
    del eng
    return _RUNS[cid]


# ---------------------------------------------------------------- 1. every embedding size, every table mode
@pytest.mark.parametrize("c", V.SIZES, ids=V.case_id)
def test_every_size_and_mode_matches_oracle(hip_lib, c):
    _run(c)


@pytest.mark.parametrize("model", ["deepfm_pipeline", "wdl"])
@pytest.mark.parametrize("E", [4, 32, 64])
def test_lazy_bit_identical_to_sorted(hip_lib, model, E):
    """The single-valued models' record path against the dense table with the sorted backward: the same
    ordered sums, so logits, parameters and first moments bit for bit (E = 8 / 16: test_gpu_parity.py)."""
    a, b = (_run((model, V.kwargs(model, E), V.B0, mode)) for mode in ("lazy", "sorted"))
    for za, zb in zip(a["zs"], b["zs"]):
        np.testing.assert_array_equal(za, zb)
    for k in a["params"]:
        np.testing.assert_array_equal(a["params"][k], b["params"][k], err_msg=k)
    for k in a["grads"]:
        np.testing.assert_array_equal(a["grads"][k], b["grads"][k], err_msg=k)


# ---------------------------------------------------------------- 2. predict paths
@pytest.mark.parametrize("model,kw", V.PREDICT, ids=lambda v: v if isinstance(v, str) else "E%d-S%d" % (v["E"], v["S"]))
def test_predict_routes_bit_identical(hip_lib, model, kw, monkeypatch):
    """predict() from the records (gather + indexed lookup), on the flushed planes (the first layer
    gathering the deep rows where it can) and with the fused gather off: the same bits, within TOL of the
    oracle on the exported parameters; the route taken is the one the shape calls for; and with
    DLAMD_GATHER_TAB=1 the table form is taken only where dl_embed_fwd_gtab_ok holds."""
    spec = ModelSpec(model, **kw)
    cfg = R.make_cfg(model, **kw)
    B = V.B0
    e = CTREngine(spec, max_batch=B, seed=3, adam="lazy")
    bs = V.batches(model, kw, B, 4, seed=29)
    for i, bt in enumerate(bs[:3]):
        e.train_step(bt, graph=i >= 1)
    fused = V.fused_gather_ok(kw)
    assert e.fused_gather_rows() == fused
    b = dict(bs[3])
    cate = np.array(b["cate_feats"], copy=True)
    cate[::9, :] = 0                         # padding ids: the zero row
    b["cate_feats"] = cate
    assert e.since_flush == 3
    calls = []
    orig = e._c
    monkeypatch.setattr(e, "_c", lambda tag, fn, *a: (calls.append(fn), orig(tag, fn, *a))[1])
    rec = e.predict(b, logits=True)          # rows lag: gather + indexed lookup, the deep rows by the first layer
    assert "dl_rec_gather" in calls and "dl_embed_fwd_indexed" in calls
    assert ("dl_gemm_s3_nt_gather_rows" in calls) == fused
    calls.clear()
    e.flush(planes=True)
    assert e.fused_gather_l0() == fused
    planes = e.predict(b, logits=True)
    assert ("dl_gemm_s3_nt_gather" in calls) == fused
    assert "dl_embed_fwd_slots" in calls or "dl_embed_fwd" in calls
    monkeypatch.setenv("DLAMD_GATHER_TAB", "1")
    calls.clear()
    tab = e.predict(b, logits=True)
    gtab = fused and V.gtab_ok(model, kw)
    assert bool(_lib.lib().dl_embed_fwd_gtab_ok(_lib.C.byref(e._flat_layout(B)))) == V.gtab_ok(model, kw)
    assert ("dl_gemm_s3_nt_gather_tab" in calls) == gtab and ("dl_embed_fwd_gtab" in calls) == gtab
    monkeypatch.setenv("DLAMD_GATHER_TAB", "0")
    monkeypatch.setenv("DLAMD_FUSED_GATHER", "0")
    assert not e.fused_gather_l0() and not e.fused_gather_rows()
    calls.clear()
    plain = e.predict(b, logits=True)
    assert not [f for f in calls if f.startswith("dl_gemm_s3_nt_gather")]
    np.testing.assert_array_equal(planes, rec)
    np.testing.assert_array_equal(tab, rec)
    np.testing.assert_array_equal(plain, rec)
    want = R.forward(cfg, e.params(), b)["z"]
    err = float(np.abs(rec - want).max())
    print("ENVELOPE_ERR predict %s E=%d S=%d fused=%s gtab=%s z=%.3g" % (model, kw["E"], kw["S"], fused, gtab, err))
    assert err <= TOL
    np.testing.assert_allclose(1.0 / (1.0 + np.exp(-rec.astype(np.float64))), e.predict(b), atol=TOL, rtol=0)


# ---------------------------------------------------------------- 3. slot-count arms
@pytest.mark.parametrize("c", V.SLOTS, ids=V.case_id)
def test_slot_count_arms_match_oracle(hip_lib, c):
    _run(c)


@pytest.mark.parametrize("model,kw", V.ONE_SLOT_MORE, ids=lambda v: v if isinstance(v, str) else "E%d" % v["E"])
def test_one_slot_more_is_refused(hip_lib, model, kw):
    """129 slots: refused when the model is described (and, for a caller that builds the layout itself,
    by the library before anything is launched: the outputs keep their sentinel)."""
    with pytest.raises(ValueError, match="too many fields"):
        ModelSpec(model, **kw)
    spec = ModelSpec(model, **dict(kw, C=14, S=57))
    eng = CTREngine(spec, max_batch=32, seed=1)
    b = V.batches(model, dict(kw, C=14, S=57), 32, 1)[0]
    eng.stage(b)
    L = eng._layout(32)
    L.cont_fields = 15                                   # one slot past the limit
    eng.x0.fill_(7.0)
    eng.fm_out.fill_(7.0)
    with pytest.raises(_lib.DLError, match="too many fields"):
        p = _lib.ptr
        _lib.call("dl_embed_fwd", _lib.C.byref(L), p(eng.table), p(eng.first), p(eng.in_cate), p(eng.in_cont),
                  p(eng.in_vec), p(eng.x0), p(eng.fm_out), p(eng.fm_sum), p(eng.err), _lib.stream_handle())
    torch.cuda.synchronize()
    assert (eng.x0 == 7.0).all() and (eng.fm_out == 7.0).all()


@pytest.mark.parametrize("E", [4, 16, 32])
def test_record_forward_past_64_fm_fields_takes_the_indexed_lookup(hip_lib, E, monkeypatch):
    """71 FM fields, past the 64 the record form of the flat lookup takes (dl_embed_fwd_rec_flat):
    predict() on a flushed table without planes (DLAMD_FLAT_PLANES=0) goes through the gather + indexed
    lookup instead of failing inside the launch, and gives the planes' bits."""
    monkeypatch.setenv("DLAMD_FLAT_PLANES", "0")
    kw = V.kwargs("deepfm_pipeline", E, C=14, S=57)
    e = CTREngine(ModelSpec("deepfm_pipeline", **kw), max_batch=64, seed=3, adam="lazy")
    assert not e.flat_planes and e.spec.F == 71
    bs = V.batches("deepfm_pipeline", kw, 64, 3)
    for bt in bs[:2]:
        e.train_step(bt)
    e.flush()
    calls = []
    orig = e._c
    monkeypatch.setattr(e, "_c", lambda tag, fn, *a: (calls.append(fn), orig(tag, fn, *a))[1])
    got = e.predict(bs[2], logits=True)
    assert "dl_embed_fwd_indexed" in calls and "dl_embed_fwd_rec_flat" not in calls
    e.flat_planes = True
    calls.clear()
    want = e.predict(bs[2], logits=True)
    assert "dl_embed_fwd_slots" in calls
    np.testing.assert_array_equal(got, want)
    # 64 fields and fewer keep the record form
    kw = V.kwargs("deepfm_pipeline", E, C=13, S=26)
    e = CTREngine(ModelSpec("deepfm_pipeline", **kw), max_batch=64, seed=3, adam="lazy")
    e.train_step(V.batches("deepfm_pipeline", kw, 64, 1)[0])
    e.flush()
    calls.clear()
    monkeypatch.setattr(e, "_c", lambda tag, fn, *a, o=e._c: (calls.append(fn), o(tag, fn, *a))[1])
    e.predict(V.batches("deepfm_pipeline", kw, 64, 1)[0])
    assert "dl_embed_fwd_rec_flat" in calls


# ---------------------------------------------------------------- 4. cont-field arms
@pytest.mark.parametrize("c", V.CONT, ids=V.case_id)
def test_cont_field_arms_match_oracle(hip_lib, c):
    _run(c)


# ---------------------------------------------------------------- 5. batch edges
@pytest.mark.parametrize("c", V.EDGE + [V.TINY], ids=V.case_id)
def test_batch_edges_match_oracle(hip_lib, c):
    _run(c)


# ---------------------------------------------------------------- 6. catch-up across the 256-step window
@pytest.mark.parametrize("model,E,hist_len", V.CATCH_UP)
def test_catch_up_past_the_window_bit_identical_to_dense(hip_lib, model, E, hist_len):
    """Rows that return after lagging 299 steps (past the 256 steps of the alpha ring the catch-up keeps in
    LDS: the older ones come from the global ring, rec.h catch_up4 / catch_up1) against the dense engine
    with the same sorted gradients: logits, table, dense parameters and Adam moments bit for bit, no
    scheduled flush in between (as test_lazy_adam_bit_identical_to_dense at an 8-entry ring)."""
    kw = V.kwargs(model, E)
    spec = ModelSpec(model, **kw)
    B, n = 64, V.LAG_STEPS
    dense = CTREngine(spec, max_batch=B, seed=3, bwd="sorted")
    lazy = CTREngine(spec, max_batch=B, seed=3, adam="lazy", hist_len=hist_len)
    same = np.testing.assert_array_equal
    bs = V.lag_batches(model, kw, B, n)
    for i, b in enumerate(bs):
        dense.train_step(b, graph=i >= 3)
        lazy.train_step(b, graph=i >= 3)
        if i in (0, 1, n - 1):
            torch.cuda.synchronize()
            same(lazy.z[:B].cpu().numpy(), dense.z[:B].cpu().numpy(), err_msg="logits step %d" % i)
    torch.cuda.synchronize()
    lazy.check_error()
    dense.check_error()
    assert lazy.since_flush == n and lazy.steps == n     # no scheduled flush: every lag is the rows' own
    pd, pl = dense.params(), lazy.params()
    for k in pd:
        same(pl[k], pd[k], err_msg=k)
    sd, sl = dense.adam_state(), lazy.adam_state()
    for k in sd:
        same(sl[k], sd[k], err_msg=k)
    dd, dl = dense.dense_state(), lazy.dense_state()
    for mv in ("m", "v"):
        for k in dd[mv]:
            same(dl[mv][k], dd[mv][k], err_msg="%s %s" % (mv, k))
    print("ENVELOPE_ERR catch_up %s E=%d hist_len=%d lag=%d: bit-identical" % (model, E, hist_len, n - 1))
