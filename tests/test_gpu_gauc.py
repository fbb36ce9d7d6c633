"""GPU checks of the eval metrics beside the pooled AUC (include/dlamd.h dl_gauc / dl_eval_stats,
deep_learning_amd/metrics.py): per-group AUC against the numpy per-group loop of
tests/_gauc_ref.py, its exactness and determinism, the log-loss / calibration sums, and the
drop-in options that ask for them."""
import numpy as np
import pytest
import torch

from tests import _gauc_ref as G

pytestmark = pytest.mark.gpu

WEIGHTINGS = ("size", "uniform")


@pytest.fixture(scope="module")
def case3():
    """The heavy-tailed case and its reference for both weightings, computed once and left unchanged."""
    y, s, g = G.case3()
    ref = {w: G.gauc(y, s, g, w) for w in WEIGHTINGS}
    n = len(y)
    # the comparison is not vacuous: most samples lie in valid groups, one group spans scan tiles
    assert ref["size"][1] >= 0.9 * n and np.bincount(g).max() > 4096
    assert ref["size"][1:] == ref["uniform"][1:]
    return y, s, g, ref


def _check(y, s, g, ref=None):
    from deep_learning_amd.metrics import group_auc
    for w in WEIGHTINGS:
        r = ref[w] if ref else G.gauc(y, s, g, w)
        v, d = group_auc(y, s, g, weighting=w, details=True)
        assert (d["covered_samples"], d["valid_groups"], d["groups"]) == r[1:], (w, d, r)
        assert abs(v - r[0]) < 1e-12, (w, v, r[0])


def test_tiny_cases_exact(hip_lib):
    from deep_learning_amd.metrics import group_auc, roc_auc
    with pytest.raises(ValueError, match="both classes"):
        group_auc([1], [0.5], [0])
    assert group_auc([0, 1], [0.2, 0.7], [5, 5]) == 1.0
    assert group_auc([0, 1], [0.7, 0.2], [5, 5]) == 0.0
    assert group_auc([0, 1], [0.4, 0.4], [5, 5]) == 0.5
    # two groups, each perfectly ranked, interleaved so that the pooled ranking is not
    y, s, g = [0, 1, 0, 1], [0.1, 0.2, 0.6, 0.7], [0, 0, 1, 1]
    assert roc_auc(y, s) < 1.0
    for w in WEIGHTINGS:
        assert group_auc(y, s, g, weighting=w) == 1.0
    # the same score in two groups does not tie across them
    v, d = group_auc([1, 0, 0, 1], [0.5, 0.2, 0.5, 0.7], [3, 3, 9, 9], details=True)
    assert v == 1.0 and d == {"covered_samples": 4, "valid_groups": 2, "groups": 2}
    # -0.0 ties with +0.0 inside a group
    assert group_auc([0, 1], np.float32([-0.0, 0.0]), [1, 1]) == 0.5
    assert group_auc([1, 0], np.float32([-0.0, 0.0]), [1, 1]) == 0.5
    # both ends of the id range are ids of their own
    v, d = group_auc([0, 1, 1, 0], [0.1, 0.9, 0.3, 0.8], [0, 0, 2 ** 31 - 1, 2 ** 31 - 1], details=True)
    assert v == 0.5 and d["groups"] == 2 and d["valid_groups"] == 2
    for bad in (-1, 2 ** 31, -2 ** 31, 2 ** 32 + 5):
        with pytest.raises(ValueError, match="group ids"):
            group_auc([0, 1, 1, 0], [0.1, 0.9, 0.3, 0.8], [5, 5, bad, 5])
    with pytest.raises(ValueError, match="length"):
        group_auc([0, 1], [0.1, 0.9], [5, 5, 5])
    with pytest.raises(ValueError, match="weighting"):
        group_auc([0, 1], [0.1, 0.9], [5, 5], weighting="sqrt")


def test_raw_call_refuses_unknown_weighting(hip_lib):
    from deep_learning_amd import _lib
    n = 4
    s = torch.rand(n, device="cuda")
    g = torch.zeros(n, dtype=torch.int64, device="cuda")
    ws = torch.empty(int(hip_lib.dl_gauc_workspace_bytes(n)), dtype=torch.uint8, device="cuda")
    out = torch.empty(4, dtype=torch.float64, device="cuda")
    with pytest.raises(_lib.DLError, match="weighting"):
        _lib.call("dl_gauc", _lib.ptr(s), 1, _lib.ptr(s), 1, _lib.ptr(g), 1, n, 2, _lib.ptr(ws), ws.numel(),
                  _lib.ptr(out), _lib.stream_handle())
    assert hip_lib.dl_gauc_workspace_bytes(0) == -1 and hip_lib.dl_gauc_workspace_bytes(2 ** 31) == -1
    assert hip_lib.dl_eval_stats_workspace_bytes(0) == -1 and hip_lib.dl_eval_stats_workspace_bytes(2 ** 31) == -1


def test_one_group_equals_roc_auc(hip_lib):
    from deep_learning_amd.metrics import group_auc, roc_auc
    rng = np.random.default_rng(11)
    n = 3 * 4096 + 5
    s = (np.round(rng.random(n) * 50) / 50).astype(np.float32)
    y = (rng.random(n) < 0.2 + 0.5 * s).astype(np.float32)
    g = np.full(n, 77, np.int64)
    want = roc_auc(y, s)
    for w in WEIGHTINGS:
        v, d = group_auc(y, s, g, weighting=w, details=True)
        assert abs(v - want) < 1e-12
        assert d == {"covered_samples": n, "valid_groups": 1, "groups": 1}


def test_random_heavy_tailed_groups(hip_lib, case3):
    y, s, g, ref = case3
    _check(y, s, g, ref)


def test_accumulator_ragged_batches_and_strided_inputs(hip_lib, case3):
    from deep_learning_amd.metrics import EvalAccumulator, group_auc, roc_auc
    y, s, g, ref = case3
    n = len(y)
    acc = EvalAccumulator()
    cuts = [0, 1, 4097, 50_000, 50_003, 131_072, n]
    for a, b in zip(cuts[:-1], cuts[1:]):
        acc.add(y[a:b].reshape(-1, 1), torch.from_numpy(s[a:b].copy()).cuda(), g[a:b])
    res = acc.results()
    assert acc.result() == res["auc"] == roc_auc(y, s)
    assert abs(res["gauc"] - ref["size"][0]) < 1e-12
    assert (res["gauc_covered"], res["gauc_groups"]) == ref["size"][1:3]
    st = G.eval_stats(y, s + np.float32(0.5))
    acc2 = EvalAccumulator(weighting="uniform")
    acc2.add(y, s + np.float32(0.5), g)
    res2 = acc2.results()
    assert abs(res2["gauc"] - ref["uniform"][0]) < 1e-12       # a shift keeps every order and tie here
    assert abs(res2["logloss"] - st["logloss"]) <= 1e-10 * st["logloss"]
    assert abs(res2["calibration"] - st["calibration"]) <= 1e-10 * st["calibration"]
    # strided: the score in column 1 of [n, 3], label and group id in columns of their own matrices
    S = torch.full((n, 3), 9.0, device="cuda")
    S[:, 1] = torch.from_numpy(s.copy()).cuda()
    Y = torch.full((n, 2), 7.0, device="cuda")
    Y[:, 0] = torch.from_numpy(y.copy()).cuda()
    Gm = torch.full((n, 4), 123, dtype=torch.int64, device="cuda")
    Gm[:, 3] = torch.from_numpy(g.copy()).cuda()
    for w in WEIGHTINGS:
        v, d = group_auc(Y[:, 0], S[:, 1], Gm[:, 3], weighting=w, details=True)
        assert abs(v - ref[w][0]) < 1e-12
        assert (d["covered_samples"], d["valid_groups"], d["groups"]) == ref[w][1:]


def test_determinism_and_permutation(hip_lib, case3):
    from deep_learning_amd.metrics import group_auc
    y, s, g, ref = case3
    ty, ts, tg = (torch.from_numpy(a.copy()).cuda() for a in (y, s, g))
    a = group_auc(ty, ts, tg)
    b = group_auc(ty, ts, tg)
    assert np.float64(a).tobytes() == np.float64(b).tobytes()
    perm = np.random.default_rng(5).permutation(len(y))
    for w in WEIGHTINGS:
        v, d = group_auc(y[perm], s[perm], g[perm], weighting=w, details=True)
        assert (d["covered_samples"], d["valid_groups"], d["groups"]) == ref[w][1:]
        assert abs(v - ref[w][0]) < 1e-12


@pytest.mark.parametrize("n", [4096, 4097])
def test_boundary_groups_of_two(hip_lib, n):
    rng = np.random.default_rng(n)
    g = rng.permutation(np.arange(n) // 2).astype(np.int64)      # every group of size 2 (4097: one of size 1)
    s = (np.round(rng.random(n) * 4) / 4).astype(np.float32)
    y = (rng.random(n) < 0.5).astype(np.float32)
    _check(y, s, g)


def test_boundary_group_edge_on_the_tile_edge(hip_lib):
    rng = np.random.default_rng(8)
    n = 8192
    g = np.repeat(np.int64([40, 41]), 4096)                      # sorted by group: the one boundary at 4096
    s = (np.round(rng.random(n) * 100) / 100).astype(np.float32)
    y = (rng.random(n) < 0.3 + 0.4 * s).astype(np.float32)
    _check(y, s, g)
    perm = rng.permutation(n)
    _check(y[perm], s[perm], g[perm])


def test_all_groups_of_size_one(hip_lib):
    from deep_learning_amd.metrics import _gauc_call, group_auc
    n = 5000
    rng = np.random.default_rng(2)
    y = (rng.random(n) < 0.5).astype(np.float32)
    s = rng.random(n).astype(np.float32)
    g = rng.permutation(n).astype(np.int64) * 3
    with pytest.raises(ValueError, match="both classes"):
        group_auc(y, s, g)
    v, covered, valid, total = _gauc_call(y, s, g, "size")
    assert v != v and (covered, valid, total) == (0, 0, n)


def test_eval_stats(hip_lib, case3):
    from deep_learning_amd.metrics import eval_stats
    y, s, g, ref = case3
    p = s + np.float32(0.5)                                      # the 1/200 grid on [0, 1], both ends included
    assert p.min() == 0.0 and p.max() == 1.0
    cases = [(y, p), (np.float32([1, 0, 0, 1, 1, 0]), np.float32([0.0, 1.0, 0.0, 1.0, 0.25, 0.5]))]
    for yy, pp in cases:
        want = G.eval_stats(yy, pp)
        assert np.isfinite(want["logloss"])
        for src in ((yy, pp), (torch.from_numpy(yy.copy()).cuda(), torch.from_numpy(pp.copy()).cuda())):
            got = eval_stats(*src)
            for k in ("logloss", "mean_score", "calibration"):
                assert abs(got[k] - want[k]) <= 1e-10 * abs(want[k]), (k, got[k], want[k])
            assert got["positive_rate"] == want["positive_rate"] and got["n"] == want["n"] == len(yy)
    assert eval_stats([0, 0], [0.25, 0.5])["calibration"] == float("inf")
    with pytest.raises(ValueError, match="length"):
        eval_stats([0, 1], [0.5])


def _conf(d):
    lines = ["f%d\tx\tfloat" % i for i in range(13)] + ["c%d\tx\tstring" % i for i in range(26)]
    (d / "dnn.conf").write_text("\n".join(lines) + "\n")


def test_dropin_eval_and_predict_options(hip_lib, tmp_path, capsys):
    from deep_learning_amd.local_run import ModelParams
    from deep_learning_amd.models import deepfm_pipeline as M
    from deep_learning_amd.models._ctr_model import export_model
    from deep_learning_amd.synthetic import make_batch
    (tmp_path / "conf").mkdir()
    _conf(tmp_path / "conf")
    V = 3000
    argv = ["local_run.py", "deepfm_pipeline", "train", "1", "8", str(V), "3", str(tmp_path / "conf"), "tr/", "pr/",
            str(tmp_path / "model_pb"), str(tmp_path / "ckpt"), "0", str(tmp_path / "ckpt"), "batch_size=64",
            "hidden_units=32,16", "shuffle=0"]
    rng = np.random.default_rng(4)
    parts = []
    for i, n in enumerate((200, 136)):
        b = make_batch(n, cate_index_size=V, seed=90 + i)
        b["cate_feats"] = b["cate_feats"].copy()
        b["cate_feats"][:, 0] = rng.integers(1, 12, n)           # slot 0: a user id with a few users
        parts.append(b)
    plain = M.DeepModel(ModelParams(argv), [], parts)
    opted = M.DeepModel(ModelParams(argv + ["gauc_slot=0", "eval_metrics=auc,gauc,logloss"]), [], parts)
    plain.model_optimizer()
    opted.model_optimizer()
    opted.engine.load_params(plain.engine.params())
    val = M.DeepModel.get_val_data(None, parts)
    capsys.readouterr()
    auc0 = plain.eval(None, val)
    assert capsys.readouterr().out == ""
    assert not hasattr(plain, "last_eval") or set(plain.last_eval) == {"auc"}
    auc1 = opted.eval(None, val)
    assert np.float64(auc0).tobytes() == np.float64(auc1).tobytes()
    assert list(opted.last_eval) == ["auc", "gauc", "logloss"] and opted.last_eval["auc"] == auc1
    # the references on the engine's own scores
    y = np.concatenate([np.asarray(b["label"]).reshape(-1) for b in parts])
    g = np.concatenate([b["cate_feats"][:, 0] for b in parts])
    from deep_learning_amd.models._ctr_model import _predict_batches
    s = np.concatenate([_predict_batches(opted.engine, b).cpu().numpy().reshape(-1) for b in parts])
    want = G.gauc(y, s, g)
    assert want[2] >= 5                                          # several users hold both classes
    assert abs(opted.last_eval["gauc"] - want[0]) < 1e-12
    ll = G.eval_stats(y, s)["logloss"]
    assert abs(opted.last_eval["logloss"] - ll) <= 1e-10 * ll
    # predict(): the reference's lines alone without options, one more line per metric with them
    export_model(plain.engine, str(tmp_path / "model_pb"))
    capsys.readouterr()
    p0 = M.predict(parts, str(tmp_path / "model_pb"))
    out0 = capsys.readouterr().out.splitlines()
    assert out0 == ["-----------end of data_set-----------", "val of auc:%.5f" % p0, "---end---"]
    p1 = M.predict(parts, str(tmp_path / "model_pb"), eval_metrics=["auc", "gauc", "logloss"], gauc_slot=0)
    out1 = capsys.readouterr().out.splitlines()
    assert p1 == p0 and abs(p0 - auc0) < 1e-5
    from deep_learning_amd.models._ctr_model import load_model
    eng = load_model(str(tmp_path / "model_pb"), max_batch=200)       # predict()'s engine: its own scores
    sp = np.concatenate([_predict_batches(eng, b).cpu().numpy().reshape(-1) for b in parts])
    assert out1 == out0[:2] + ["val of gauc:%.5f" % G.gauc(y, sp, g)[0],
                               "val of logloss:%.5f" % G.eval_stats(y, sp)["logloss"]] + out0[2:]
    assert sum("val of auc:" in l for l in out1) == 1
    with pytest.raises(ValueError, match="gauc_slot"):
        M.predict(parts, str(tmp_path / "model_pb"), eval_metrics=["gauc"])
    # fit(): the val_auc line as it was, followed by one line of the requested fields
    train = [make_batch(64, cate_index_size=V, seed=i) for i in range(3)]
    for m in (plain, opted):
        m.data_dict = train
        m.fit(1, parts)
    lines = capsys.readouterr().out.splitlines()
    evals = [i for i, l in enumerate(lines) if "val_auc:" in l]
    assert len(evals) == 4 and not any("val_gauc" in l for l in lines[:evals[2]])    # two evals per fit
    for i, step in zip(evals[2:], (1, 2)):
        assert lines[i].startswith("[%d] val_auc:" % step) and "\t loss:" in lines[i] and "gauc" not in lines[i]
        assert lines[i + 1].startswith("[%d] val_gauc:" % step) and " val_logloss:" in lines[i + 1]
    # last_eval is the last evaluation's: the line after step 2's
    assert lines[evals[3] + 1] == "[2] val_gauc:%s val_logloss:%s" % (opted.last_eval["gauc"],
                                                                       opted.last_eval["logloss"])
    assert sum("val_gauc" in l for l in lines) == 2
