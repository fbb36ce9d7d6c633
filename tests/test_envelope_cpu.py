"""The envelope tests' fixtures, checked without a GPU (tests/_envelope.py): the case tables reach every
arm of the lookup dispatch they are there for, every ModelSpec constructs or is refused where stated,
and every gradient fixture is well enough conditioned that the GPU file's REL bound measures the
kernels: the oracle's own float32 backward within REL / 4 of its float64 one, and no first-step
pre-activation within RELU_MARGIN of zero (a ReLU decided the other way in float32 moves a whole column
of a weight gradient)."""
import numpy as np
import pytest

from deep_learning_amd.engine import ModelSpec
from tests import _envelope as V


def _arms(cases, **kw):
    return {V.fwd_arm(m, k, **kw) for m, k, _, _ in cases}


def test_size_cases_cover_every_model_size_and_mode():
    got = {(m, k["E"], mode) for m, k, _, mode in V.SIZES}
    for m in ("deepfm_pipeline", "wdl", "deepfm_multi_cate"):
        for E in (4, 32, 64):
            for mode in ("atomic", "sorted", "lazy"):
                assert (m, E, mode) in got
    for m in ("dnn_pipeline", "dnn_multi"):
        for E in (4, 32, 64):
            assert (m, E, "lazy") in got
    assert _arms(V.SIZES) >= {(4, 2), (32, 16), (64, 32)}
    # the atomic backward: 16 rows a wave instruction at E = 4 (2 passes over the cont rows), 1 at E = 64 (32)
    assert {V.bwd_passes(k) for m, k, _, mode in V.SIZES if mode == "atomic"} >= {(16, 2), (2, 16), (1, 32)}


def test_slot_cases_reach_every_forward_arm():
    arms = _arms(V.SLOTS)
    assert arms >= {(16, 6), (16, 7), (16, 8), (8, 4), (4, 2), (32, 16), (64, 32)}
    by_shape = {(k["E"], k["C"], k["S"]): V.slots(m, k) for m, k, _, _ in V.SLOTS}
    assert by_shape == {(16, 13, 40): 93, (16, 13, 48): 109, (16, 13, 57): 127, (16, 14, 57): 128, (8, 13, 48): 109,
                        (4, 14, 57): 128, (32, 14, 57): 128, (64, 14, 50): 114, (64, 13, 128): 128}
    # the limit itself at every E whose all-slots form it bounds
    assert {k["E"] for m, k, _, _ in V.SLOTS if V.slots(m, k) == V.MAX_SLOTS} == {4, 16, 32, 64}
    assert V.fwd_arm("dnn_pipeline", V.kwargs("dnn_pipeline", 64, S=128)) == (64, 32)
    assert {V.fwd_arm(m, k) for m, k, _, _ in V.SLOTS if (k["C"], k["S"]) == (13, 40)} == {(16, 6)}
    assert {V.fwd_arm(m, k) for m, k, _, _ in V.SLOTS if (k["E"], k["S"]) == (16, 48)} == {(16, 7)}
    assert {V.fwd_arm(m, k) for m, k, _, _ in V.SLOTS if (k["E"], k["C"], k["S"]) == (16, 13, 57)} == {(16, 8)}
    # the lazy forward that leaves the deep rows to the first layer looks up the FM slots only
    assert V.fwd_arm("deepfm_pipeline", V.kwargs("deepfm_pipeline", 16, C=13, S=40), deep=False) == (16, 4)
    for m, k, _, _ in V.SLOTS:
        assert V.limit_slots(m, k) <= V.MAX_SLOTS
        assert {mode for m2, k2, _, mode in V.SLOTS if k2 == k} == {"atomic", "lazy"}
    # more than the record forward's 64 FM fields at S = 57
    assert sum(V.slots(m, k, deep=False) > 64 for m, k, _, mode in V.SLOTS if mode == "lazy") == 4
    # E = 64: the widest shape the output layer takes (FM fields + E = 128 columns), every pass of the
    # all-slots form but the last three holding a row
    e64 = V.kwargs("deepfm_pipeline", 64, C=14, S=50)
    assert V.slots("deepfm_pipeline", e64, deep=False) + 64 == V.MAX_FM_COLS and -(-V.slots("deepfm_pipeline", e64) // 4) == 29
    for m, k in V.ONE_SLOT_MORE:
        assert V.limit_slots(m, k) == V.MAX_SLOTS + 1
    # every test elsewhere stays at or below NPS 5 (S <= 26: 65 slots at E = 16)
    assert V.fwd_arm("deepfm_pipeline", V.kwargs("deepfm_pipeline", 16)) == (16, 5)


def test_cont_cases_reach_both_register_forms():
    fm = [(m, k, B, mode) for m, k, B, mode in V.CONT if m == "deepfm_pipeline"]
    for E in (4, 16, 64):
        for mode in ("sorted", "lazy"):
            got = {(k["C"], V.cont_arm(m, k)) for m, k, _, md in fm if k["E"] == E and md == mode}
            assert got == {(16, (16, 4)), (17, (32, 1)), (32, (32, 1))}
        assert {k["C"] for m, k, _, md in fm if k["E"] == E and md == "atomic"} == {16, 17, 32}
    assert {k["C"] for _, k in V.ONE_CONT_MORE} == {V.MAX_FM_CONT + 1}
    wide = [k for m, k, _, _ in V.CONT if m == "dnn_pipeline"]
    assert wide and all(k["C"] > 64 and k["V"] > 64 and k["E"] == 32 for k in wide)


def test_batch_cases_cross_the_tile_and_grid_edges():
    Bs = {(k["E"], B) for m, k, B, mode in V.EDGE if mode == "lazy"}
    assert Bs >= {(E, B) for E in (4, 64) for B in (1, V.TILE - 1, V.TILE, V.TILE + 1)}
    big = [(k["E"], B) for m, k, B, mode in V.EDGE if mode == "atomic"]
    assert sorted(big) == [(4, 4133), (64, 4133)] and all(V.bwd_wave_wraps(B) for _, B in big)
    assert not V.bwd_wave_wraps(V.B0) and not V.fwd_tile_wraps(65536)   # the full-size test: 4,096 tiles
    assert V.fwd_tile_wraps(V.TINY[2]) and V.TINY[2] % V.TILE == 1


def test_predict_cases_sit_on_both_sides_of_every_route():
    route = {(m, k["E"], k["S"]): (V.fused_gather_ok(k), V.gtab_ok(m, k)) for m, k in V.PREDICT}
    for m in ("deepfm_pipeline", "dnn_pipeline"):
        assert route[(m, 4, 26)] == (False, False)
        assert route[(m, 32, 26)] == (True, False) and route[(m, 64, 26)] == (True, False)
        assert route[(m, 16, 40)][0] and not route[(m, 16, 42)][0]
    assert route[("dnn_pipeline", 16, 40)] == (True, True)


def test_catch_up_cases_lag_past_the_window():
    assert V.LAG_STEPS - 1 > V.HIST_WIN
    for model, E, hist_len in V.CATCH_UP:
        assert V.LAG_STEPS < hist_len - 2       # no scheduled flush (CTREngine.train_step)
        kw = V.kwargs(model, E)
        bs = V.lag_batches(model, kw, 64, n=4)
        C = kw["C"] if model in V.FM_CONT else 0
        lo = set(np.unique(bs[0]["cate_feats"])) | set(np.unique(bs[0]["cate_feats"] + C))
        lo |= set(np.unique(bs[3]["cate_feats"])) | set(np.unique(bs[3]["cate_feats"] + C))
        hi = set(np.unique(bs[1]["cate_feats"])) | set(np.unique(bs[1]["cate_feats"] + C))
        hi |= set(np.unique(bs[2]["cate_feats"])) | set(np.unique(bs[2]["cate_feats"] + C))
        sp = ModelSpec(model, **kw)
        assert not lo & hi and max(hi) < sp.n_rows and min(lo | hi) >= 0
        assert set(np.unique(bs[0]["cate_feats"])) & set(np.unique(bs[3]["cate_feats"]))   # rows do return
        if "wide_feats" in bs[0]:
            wlo = set(np.unique(bs[0]["wide_feats"])) | set(np.unique(bs[3]["wide_feats"]))
            whi = set(np.unique(bs[1]["wide_feats"])) | set(np.unique(bs[2]["wide_feats"]))
            assert not wlo & whi and wlo & set(np.unique(bs[3]["wide_feats"])) & set(np.unique(bs[0]["wide_feats"]))
            assert min(wlo | whi) >= 0 and max(wlo | whi) < sp.n_rows + sp.hidden[-1]   # wdl_weights' rows
    assert {(m, E) for m, E, h in V.CATCH_UP if h == 4096} == {("deepfm_pipeline", 16), ("deepfm_pipeline", 4),
                                                               ("wdl", 16)}
    assert any(h == 512 for _, _, h in V.CATCH_UP)


@pytest.mark.parametrize("c", V.GRADIENT_CASES, ids=V.case_id)
def test_spec_constructs(c):
    model, kw, B, mode = c
    sp = ModelSpec(model, **kw)
    assert sp.E == kw["E"] and sp.S == kw["S"]
    assert sp.F == V.slots(model, kw, deep=False) + (sp.M if sp.fm else 0)


@pytest.mark.parametrize("model,kw", V.PREDICT, ids=lambda v: v if isinstance(v, str) else "E%d-S%d" % (v["E"], v["S"]))
def test_predict_spec_constructs(model, kw):
    ModelSpec(model, **kw)


@pytest.mark.parametrize("model,kw", V.ONE_SLOT_MORE, ids=lambda v: v if isinstance(v, str) else "E%d" % v["E"])
def test_one_slot_more_is_refused_at_construction(model, kw):
    with pytest.raises(ValueError, match="too many fields"):
        ModelSpec(model, **kw)
    ModelSpec(model, **dict(kw, C=14, S=57))                      # the limit itself
    with pytest.raises(ValueError, match="too many fields"):      # without an FM part: the deep slots alone
        ModelSpec("dnn_pipeline", **dict(kw, S=129))
    ModelSpec("dnn_pipeline", **dict(kw, S=128))


@pytest.mark.parametrize("model,kw", V.HEAD_REFUSED, ids=lambda v: v if isinstance(v, str) else "S%d" % v["S"])
def test_more_fm_columns_than_the_head_takes_is_refused_at_construction(model, kw):
    """FM fields + E past the output layer's 128 columns (csrc/head.hip): ModelSpec used to accept the
    shape and the first step failed inside the head's launch (E = 64 at the 128-slot limit: 135 columns)."""
    assert V.limit_slots(model, kw) <= V.MAX_SLOTS
    with pytest.raises(ValueError, match="too many FM columns"):
        ModelSpec(model, **kw)
    sp = ModelSpec(model, **dict(kw, S=kw["S"] - (7 if kw["S"] == 57 else 1)))
    assert sp.fm_cols == V.MAX_FM_COLS
    ModelSpec("dnn_pipeline", **dict(kw, C=14, multi_ranges=()))      # no FM part: no such limit


@pytest.mark.parametrize("model,kw", V.ONE_CONT_MORE, ids=lambda v: v if isinstance(v, str) else "E%d" % v["E"])
def test_one_cont_field_more_is_refused_at_construction(model, kw):
    with pytest.raises(ValueError, match="at most 32 FM cont fields"):
        ModelSpec(model, **kw)
    ModelSpec(model, **dict(kw, C=32))
    ModelSpec("dnn_pipeline", **kw)                               # cont fields outside an FM part: no limit
    ModelSpec("wdl", **dict(kw, Fw=4))


def test_tiny_case_constructs_and_its_float32_logits_hold():
    model, kw, B, _ = V.TINY
    assert ModelSpec(model, **kw).deep_in == 10 and V.TINY not in V.GRADIENT_CASES
    ref = V.case_reference(V.TINY)
    assert len(ref["zs"]) == 1
    assert float(np.abs(ref["fw0"]["z"] - ref["fw64"]["z"]).max()) < V.TOL / 4


_SEEN = set()


@pytest.mark.parametrize("c", V.GRADIENT_CASES, ids=V.case_id)
def test_gradient_fixture_is_well_conditioned(c):
    """The oracle's float32 backward within REL / 4 of its float64 one on every parameter, its float32
    logits within TOL / 4, and every pre-activation clear of zero.  (Cases that differ only in the table
    mode share one fixture: checked once.)"""
    model, kw, B, _ = c
    key = V._key(model, kw, B, V.n_steps(c), 0)
    if key in _SEEN:
        return
    _SEEN.add(key)
    ref = V.case_reference(c)
    err = V.grad_errors(ref["G32"], ref["G64"])
    worst = max(err.values())
    dz = float(np.abs(ref["fw0"]["z"] - ref["fw64"]["z"]).max())
    print("ENVELOPE_FIXTURE %s grad32=%.3g z32=%.3g margin=%.3g" % (V.case_id(c), worst, dz, ref["margin"]))
    assert worst < V.REL / 4, err
    assert dz < V.TOL / 4
    assert ref["margin"] >= V.RELU_MARGIN
    # the gradient reaches every kind of row the GPU check reads: touched rows, and rows left at exactly 0
    # (the same arrays and the same two assertions as test_gpu_envelope._run makes)
    cfg = ref["cfg"]
    for k in (V.R.table_key(cfg),) + ((V.R.first_key(cfg),) if V.R.is_fm(cfg) else ()):
        g64 = ref["G64"][k]
        touched = np.abs(g64).reshape(g64.shape[0], -1).max(1) > 0
        assert touched.any() and not touched.all(), k
    if cfg.model == "wdl":   # the wide rows no sample names: the L2 term alone, and some such row exists
        w = ref["P0"]["wdl_weights"].astype(np.float64)
        assert (ref["G64"]["wdl_weights"] == cfg.l2 * w).any()
