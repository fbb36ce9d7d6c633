"""CPU checks of the deep tower's dropout (include/dlamd.h "Dropout"): the numpy restatement of
the mask against Philox-4x32-10's known answers, the float64 autograd restatement of dnn_cate
against the oracle, ModelSpec's validation and the CLI override."""
import os

import numpy as np
import pytest

from deep_learning_amd.synthetic import make_batch
from oracle import ctr_ref as R
from tests import _dropout_ref as D


def _words(ctr, key):
    return ["%08x" % int(w) for w in D.philox4x32_10([np.array(c, np.uint64) for c in ctr], key)]


def test_philox_known_answers():
    """Random123's kat_vectors for philox4x32 10: zero, all-ones and the pi-digit inputs."""
    assert _words([0, 0, 0, 0], (0, 0)) == ["6627e8d5", "e169c58d", "bc57ac4c", "9b00dbd8"]
    f = 0xFFFFFFFF
    assert _words([f, f, f, f], (f, f)) == ["408f276d", "41c83b0e", "a20bc7c6", "6d5451fd"]
    assert _words([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], (0xA4093822, 0x299F31D0)) == \
        ["d16cfe09", "94fdcceb", "5001e420", "24126ea1"]


def test_mask_zero_counter_is_the_known_answer():
    """Element (0, 0..3) of layer 0 at step 0 under seed 0 is the zero-counter known answer
    against the threshold."""
    ka = np.array([0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8], np.uint64)
    for keep in (0.3, 0.5, 0.7, 0.9, 1.0):
        m = D.keep_mask(0, 0, 0, 1, 4, keep)
        assert m.tolist() == [(ka < D.keep_thr(keep)).tolist()]
    assert D.keep_thr(1.0) == 2 ** 32 - 1 and D.keep_thr(0.5) == 2 ** 31


def test_mask_depends_on_seed_step_layer_and_is_ragged_consistent():
    base = D.keep_mask(2019, 1, 1, 300, 230, 0.8)
    assert base.shape == (300, 230) and base.dtype == bool
    for other in (D.keep_mask(2020, 1, 1, 300, 230, 0.8), D.keep_mask(2019, 2, 1, 300, 230, 0.8),
                  D.keep_mask(2019, 1, 2, 300, 230, 0.8), D.keep_mask(2019 + (1 << 32), 1, 1, 300, 230, 0.8)):
        assert 0.25 < (other != base).mean() < 0.40      # independent masks differ on 2 * 0.8 * 0.2 = 0.32
    # the mask of a narrower or shorter tensor is the corner of the wider one's (x0 and dx0 share it)
    assert np.array_equal(D.keep_mask(2019, 1, 1, 120, 97, 0.8), base[:120, :97])
    # a lower keep drops a superset
    assert not (D.keep_mask(2019, 1, 1, 300, 230, 0.5) & ~base).any()


def test_kept_share_is_binomial():
    """300 x 230 elements at keep 0.8: within 5 binomial standard deviations (fixed seed)."""
    n = 300 * 230
    share = D.keep_mask(2019, 1, 1, 300, 230, 0.8).mean()
    assert abs(share - 0.8) < 5 * np.sqrt(0.8 * 0.2 / n)
    assert D.keep_mask(2019, 1, 1, 64, 50, 1.0).mean() > 0.999   # thr 2^32 - 1: all but a 2^-32 share kept


KW = dict(S=6, E=8, cate_index_size=500, hidden=[20, 12, 8])


def test_fp64_restatement_matches_oracle_without_dropout():
    """All-ones masks: the autograd restatement equals the oracle's forward and analytic backward
    in float64 to 1e-10 — logits, loss, every parameter's gradient, and the stage gradients."""
    cfg = R.make_cfg("dnn_cate", **KW)
    P = R.init_params(cfg, np.random.default_rng(3))
    B = 37
    b = make_batch(B, cont=0, cate_fields=KW["S"], cate_index_size=KW["cate_index_size"], seed=5, cate_only=True)
    b["cate_feats"][0, :2] = [0, 1]      # the zero row
    dims = [KW["S"] * KW["E"]] + KW["hidden"]
    ref = D.dnn_cate_fp64(cfg, P, b, [np.ones((B, d), bool) for d in dims], [1.0] * len(dims))
    fw = R.forward(cfg, P, b, dtype=np.float64)
    trace = {}
    G, _ = R.backward(cfg, P, b, fw, dtype=np.float64, trace=trace)
    np.testing.assert_allclose(ref["z"], fw["z"], rtol=0, atol=1e-10)
    assert abs(ref["loss"] - fw["loss"]) < 1e-10
    for k in P:
        np.testing.assert_allclose(ref["G"][k], G[k], rtol=0, atol=1e-10, err_msg=k)
    for i in range(len(KW["hidden"])):
        np.testing.assert_allclose(ref["dh"][i], trace["g"][i], rtol=0, atol=1e-10)
    # dropping changes the result (the restatement does use its masks)
    masks = [D.keep_mask(1, 1, l, B, d, 0.7) for l, d in enumerate(dims)]
    drop = D.dnn_cate_fp64(cfg, P, b, masks, [D.inv_keep(0.7)] * len(dims))
    assert np.abs(drop["z"] - fw["z"]).max() > 1e-3
    assert np.all(drop["dx0"][~masks[0]] == 0)


def test_modelspec_validation():
    from deep_learning_amd.engine import ModelSpec
    mk = lambda k: ModelSpec("dnn_cate", dropout_keep_deep=k, **KW)
    assert mk(None).dropout_keep_deep is None and mk(None).dropout is None
    assert mk([1, 1, 1, 1]).dropout is None and mk([1, 1, 1, 1]).dropout_keep_deep == [1.0] * 4
    assert mk((0.9, 0.8, 0.8, 0.7)).dropout == [0.9, 0.8, 0.8, 0.7]
    # the reference's default holds 5 entries for 3 layers: truncated
    assert mk([1, 0.8, 0.8, 0.8, 0.5]).dropout == [1.0, 0.8, 0.8, 0.8]
    assert mk([1, 1, 1, 1, 0.5]).dropout is None
    for bad in ([0.8, 0.8, 0.8], [], [0.0, 1, 1, 1], [1, 1.2, 1, 1], [1, -0.5, 1, 1], [1, float("nan"), 1, 1]):
        with pytest.raises(ValueError, match="dropout_keep_deep"):
            mk(bad)


def test_local_run_override(tmp_path):
    from deep_learning_amd.local_run import ModelParams
    from deep_learning_amd.models._ctr_model import _spec_from_args
    with open(os.path.join(str(tmp_path), "dnn.conf"), "w") as f:
        f.write("\n".join(["f%d\tx\tfloat" % i for i in range(13)] + ["c%d\tx\tstring" % i for i in range(26)]) + "\n")
    argv = ["local_run.py", "deepfm_pipeline", "train", "1", "8", "3000", "10", str(tmp_path), "tr/", "pr/", "pb", "ck",
            "0", "ck", "hidden_units=32,16,8"]
    mp = ModelParams(argv)
    assert mp.dropout_keep_deep == [1, 1, 1, 1, 1]                     # local_run.py:40
    assert _spec_from_args("deepfm_pipeline", mp).dropout is None
    mp = ModelParams(argv + ["dropout_keep_deep=1,0.8,0.8,0.75"])
    assert mp.dropout_keep_deep == [1.0, 0.8, 0.8, 0.75]
    assert _spec_from_args("deepfm_pipeline", mp).dropout == [1.0, 0.8, 0.8, 0.75]
    with pytest.raises(ValueError, match="dropout_keep_deep"):
        _spec_from_args("deepfm_pipeline", ModelParams(argv + ["dropout_keep_deep=0.8,0.8"]))
