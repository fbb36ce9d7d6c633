"""CPU checks of the FM part's dropout (include/dlamd.h "Dropout", dropout_keep_fm): ModelSpec's
validation, the CLI override, the sharded refusal, the masks' bit layout, and the float64
autograd restatement of deepfm_pipeline / deepfm_multi_cate against the oracle."""
import os
import types

import numpy as np
import pytest

from deep_learning_amd.synthetic import make_batch
from oracle import ctr_ref as R
from tests import _dropout_ref as D
from tests import _fm_dropout_ref as FD

KWA = dict(C=13, S=50, E=8, cate_index_size=5000, hidden=[40, 24])
KWC = dict(V=4, S=8, E=16, cate_index_size=6000, hidden=[48, 32], multi_ranges=[[0, 30, "a"], [30, 50, "b"]])


def test_modelspec_validation():
    from deep_learning_amd.engine import ModelSpec
    mk = lambda k, model="deepfm_pipeline", kw=KWA: ModelSpec(model, dropout_keep_fm=k, **kw)
    assert mk(None).dropout_keep_fm is None
    assert mk((0.7, 0.6)).dropout_keep_fm == [0.7, 0.6]
    assert mk([1, 0.8]).dropout_keep_fm == [1.0, 0.8]
    assert mk([0.9, 0.8, 0.5, 0.1]).dropout_keep_fm == [0.9, 0.8]      # a longer list is truncated
    assert mk([1, 1]).dropout_keep_fm is None and mk([1, 1, 0.5]).dropout_keep_fm is None
    # models without an FM part never read it (but a malformed list is still an error)
    dnn = dict(S=6, E=8, cate_index_size=500, hidden=[20, 12])
    assert mk((0.7, 0.6), "dnn_cate", dnn).dropout_keep_fm is None
    assert mk((0.7, 0.6), "wdl", dict(C=13, S=26, E=8, cate_index_size=3000, hidden=[40, 24], Fw=26)) \
        .dropout_keep_fm is None
    assert mk((0.7, 0.6), "deepfm_multi_cate", KWC).dropout_keep_fm == [0.7, 0.6]
    for bad in ([0.8], [], [0.0, 1], [1, 1.2], [-0.5, 1], [1, float("nan")]):
        with pytest.raises(ValueError, match="dropout_keep_fm"):
            mk(bad)
    # it is the last keyword, beside dropout_keep_deep
    sp = ModelSpec("deepfm_pipeline", dropout_keep_deep=(1, 0.8, 0.8), dropout_keep_fm=(0.9, 0.8), **KWA)
    assert sp.dropout == [1.0, 0.8, 0.8] and sp.dropout_keep_fm == [0.9, 0.8]


def test_local_run_override(tmp_path):
    from deep_learning_amd.local_run import ModelParams
    from deep_learning_amd.models._ctr_model import _spec_from_args
    with open(os.path.join(str(tmp_path), "dnn.conf"), "w") as f:
        f.write("\n".join(["f%d\tx\tfloat" % i for i in range(13)] + ["c%d\tx\tstring" % i for i in range(26)]) + "\n")
    argv = ["local_run.py", "deepfm_pipeline", "train", "1", "8", "3000", "10", str(tmp_path), "tr/", "pr/", "pb", "ck",
            "0", "ck", "hidden_units=32,16,8"]
    mp = ModelParams(argv)
    assert mp.dropout_keep_fm == [1, 1]                      # deepfm_pipeline.py:31
    assert _spec_from_args("deepfm_pipeline", mp).dropout_keep_fm is None
    mp = ModelParams(argv + ["dropout_keep_fm=0.9,0.8", "dropout_keep_deep=1,0.8,0.8,0.75"])
    assert mp.dropout_keep_fm == [0.9, 0.8]
    sp = _spec_from_args("deepfm_pipeline", mp)
    assert sp.dropout_keep_fm == [0.9, 0.8] and sp.dropout == [1.0, 0.8, 0.8, 0.75]
    with pytest.raises(ValueError, match="dropout_keep_fm"):
        _spec_from_args("deepfm_pipeline", ModelParams(argv + ["dropout_keep_fm=0.8"]))


def test_sharded_engine_refuses():
    from deep_learning_amd.engine import ModelSpec
    from deep_learning_amd.shard import ShardedCTREngine
    pk = dict(C=13, S=26, E=8, cate_index_size=3000, hidden=[40, 24])
    with pytest.raises(ValueError, match="dropout_keep_fm"):
        ShardedCTREngine(ModelSpec("deepfm_pipeline", dropout_keep_fm=(0.9, 0.8), **pk), 64,
                         types.SimpleNamespace(world=1, rank=0))


def test_masks_and_bit_layout():
    """The two masks are keep_mask under their own layer ids; a keep of 1 keeps everything; the
    packed words put column c at bit c & 63 of word c >> 6 (shape A: column 63 ends word 0)."""
    B, F, E = 5, 63, 8
    m1, m2 = FD.fm_masks(77, 3, B, F, E, (0.7, 0.6))
    assert np.array_equal(m1, D.keep_mask(77, 3, 1 << 16, B, F, 0.7))
    assert np.array_equal(m2, D.keep_mask(77, 3, (1 << 16) + 1, B, E, 0.6))
    assert FD.fm_masks(77, 3, B, F, E, (1.0, 0.6))[0].all()
    w = FD.pack_keep(m1, m2)
    assert w.shape == (B, 2) and w.dtype == np.uint64
    for b in range(B):
        for c in range(128):
            want = (m1[b, c] if c < F else m2[b, c - F]) if c < F + E else False
            assert bool((int(w[b, c >> 6]) >> (c & 63)) & 1) == bool(want), (b, c)


def _batch_a(seed, B):
    b = make_batch(B, cont=KWA["C"], cate_fields=KWA["S"], cate_index_size=KWA["cate_index_size"], seed=seed)
    b["cate_feats"][0, :2] = [0, 1]      # the zero row, an id next to it
    return b


def _batch_c(seed, B):
    b = make_batch(B, cont=0, vector=KWC["V"], cate_fields=KWC["S"], cate_index_size=KWC["cate_index_size"],
                   seed=seed, cate_only=True)
    rng = np.random.default_rng(seed + 100)
    multi = rng.integers(1, KWC["cate_index_size"], size=(B, 50))
    multi[rng.random((B, 50)) < 0.5] = 0
    multi[0, :30] = 0                    # an empty slot: div_no_nan
    b["cate_feats"] = np.concatenate([b["cate_feats"], multi], 1)
    return b


@pytest.mark.parametrize("model,kw,mk", [("deepfm_pipeline", KWA, _batch_a), ("deepfm_multi_cate", KWC, _batch_c)])
def test_fp64_restatement_matches_oracle_without_dropout(model, kw, mk):
    """All-ones masks: the autograd restatement equals the oracle's forward and analytic backward
    in float64 to 1e-10; with masks the dropped columns' first-order gradient is gone."""
    cfg = R.make_cfg(model, **kw)
    P = R.init_params(cfg, np.random.default_rng(3))
    B = 41
    b = mk(5, B)
    F, E = R.fm_fields(cfg), cfg.E
    ones = (np.ones((B, F), bool), np.ones((B, E), bool))
    ref = FD.deepfm_fp64(cfg, P, b, *ones, 1.0, 1.0)
    fw = R.forward(cfg, P, b, dtype=np.float64)
    G, _ = R.backward(cfg, P, b, fw, dtype=np.float64)
    np.testing.assert_allclose(ref["z"], fw["z"], rtol=0, atol=1e-10)
    assert abs(ref["loss"] - fw["loss"]) < 1e-10
    for k in P:
        np.testing.assert_allclose(ref["G"][k], np.asarray(G[k]).reshape(ref["G"][k].shape), rtol=0, atol=1e-10,
                                   err_msg=k)
    m1, m2 = FD.fm_masks(1, 1, B, F, E, (0.7, 0.6))
    drop = FD.deepfm_fp64(cfg, P, b, m1, m2, D.inv_keep(0.7), D.inv_keep(0.6))
    assert np.abs(drop["z"] - fw["z"]).max() > 1e-3
    # a head weight whose column is dropped in every sample would get no gradient: column sums
    gw = drop["G"]["deep_fm_weight"][:F, 0]
    assert np.all(gw[~m1.any(0)] == 0)
