"""CPU checks of the eval metrics' reference (tests/_gauc_ref.py) and of the drop-in options that
ask for them (local_run.py gauc_slot= / eval_metrics=)."""
import numpy as np
import pytest

from tests import _gauc_ref as G


def test_reference_equals_per_group_sklearn():
    from sklearn.metrics import roc_auc_score
    rng = np.random.default_rng(3)
    n = 400
    g = rng.integers(0, 25, n)
    s = (np.round(rng.random(n) * 10) / 10).astype(np.float32)       # an 11-value grid: ties in every group
    y = (rng.random(n) < 0.4).astype(np.float32)
    g[:3], y[:3] = 1000, 1                                           # a single-class group and
    g[3] = 2000                                                      # a group of one: both left out
    for weighting in ("size", "uniform"):
        num = den = 0.0
        covered = valid = 0
        for k in np.unique(g):
            m = g == k
            if len(np.unique(y[m])) < 2:
                continue
            w = m.sum() if weighting == "size" else 1
            num += w * roc_auc_score(y[m], s[m].astype(np.float64))
            den += w
            covered += int(m.sum())
            valid += 1
        got = G.gauc(y, s, g, weighting)
        assert abs(got[0] - num / den) < 1e-12
        assert got[1:] == (covered, valid, len(np.unique(g)))
        assert valid < len(np.unique(g)) and covered < n
    assert np.isnan(G.gauc([1, 0, 1], [.1, .2, .3], [0, 1, 2])[0])


def test_reference_eval_stats():
    st = G.eval_stats([1, 0, 1, 0], np.float32([1.0, 0.0, 0.5, 0.25]))
    want = -(np.log(1 + 1e-7) + np.log(1 + 1e-7) + np.log(0.5 + 1e-7) + np.log(0.75 + 1e-7)) / 4
    assert abs(st["logloss"] - want) < 1e-15 and np.isfinite(st["logloss"])
    assert st["calibration"] == 1.75 / 2 and st["mean_score"] == 1.75 / 4 and st["positive_rate"] == 0.5
    assert st["n"] == 4


def _argv(tmp_path, *over):
    conf = tmp_path / "conf"
    if not conf.exists():
        conf.mkdir()
        lines = ["f%d\tx\tfloat" % i for i in range(13)] + ["c%d\tx\tstring" % i for i in range(26)]
        (conf / "dnn.conf").write_text("\n".join(lines) + "\n")
    return ["local_run.py", "deepfm_pipeline", "train", "1", "8", "3000", "3", str(conf), "tr/", "pr/", "pb", "ck",
            "0", "ck", "batch_size=64"] + list(over)


def test_model_params_parses_eval_options(tmp_path):
    from deep_learning_amd.local_run import ModelParams
    mp = ModelParams(_argv(tmp_path, "gauc_slot=3", "eval_metrics=auc,gauc,logloss,calibration"))
    assert mp.gauc_slot == 3 and mp.eval_metrics == ["auc", "gauc", "logloss", "calibration"]
    assert mp.cate_field_size == 26
    mp = ModelParams(_argv(tmp_path, "eval_metrics=logloss"))
    assert mp.eval_metrics == ["logloss"] and not hasattr(mp, "gauc_slot")
    mp = ModelParams(_argv(tmp_path, "gauc_slot=25"))           # the last slot; a slot alone asks for nothing
    assert mp.gauc_slot == 25 and not hasattr(mp, "eval_metrics")


def test_model_params_refuses_gauc_without_slot(tmp_path):
    from deep_learning_amd.local_run import ModelParams
    with pytest.raises((SystemExit, ValueError), match="gauc_slot"):
        ModelParams(_argv(tmp_path, "eval_metrics=auc,gauc"))
    with pytest.raises((SystemExit, ValueError), match="eval_metrics"):
        ModelParams(_argv(tmp_path, "eval_metrics=auc,ndcg"))


@pytest.mark.parametrize("slot", [-1, 26, 1000])
def test_model_params_refuses_slot_out_of_range(tmp_path, slot):
    from deep_learning_amd.local_run import ModelParams
    with pytest.raises((SystemExit, ValueError), match="gauc_slot"):
        ModelParams(_argv(tmp_path, "gauc_slot=%d" % slot, "eval_metrics=gauc"))


def test_model_params_keys_unchanged_without_the_options(tmp_path):
    """The start-up dump prints ModelParams.__dict__: without the two options it has the keys it
    has with any other known override, and the options add exactly their own."""
    from deep_learning_amd.local_run import ModelParams
    plain = ModelParams(_argv(tmp_path))
    other = ModelParams(_argv(tmp_path, "learning_rate=0.01"))
    assert list(plain.__dict__) == list(other.__dict__)
    assert "gauc_slot" not in plain.__dict__ and "eval_metrics" not in plain.__dict__
    both = ModelParams(_argv(tmp_path, "gauc_slot=0", "eval_metrics=auc,gauc"))
    assert set(both.__dict__) - set(plain.__dict__) == {"gauc_slot", "eval_metrics"}
    assert {k: v for k, v in both.__dict__.items() if k in plain.__dict__} == plain.__dict__


def test_ctr_model_eval_options():
    from deep_learning_amd.models._ctr_model import _eval_options
    assert _eval_options(None, None) == ([], None)
    assert _eval_options(["auc"], 3) == ([], None)
    assert _eval_options(["auc", "gauc", "logloss"], 0) == (["gauc", "logloss"], 0)
    with pytest.raises(ValueError, match="gauc_slot"):
        _eval_options(["gauc"], None)
