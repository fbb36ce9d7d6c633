"""The engine-level GPU checks every side option of the dnn tower shares, once, over the table in
tests/_side_options.py (one Case per option, in deep_learning_amd/branches.py's order): five-step
trajectories against the option's own float64 restatement in every table mode, beside the other options,
with dropout in the tower and with sample weights; same-seed runs; refused parameters; predict, checkpoint,
export and local_run; and the unchanged kernel sequence with the option off.  An option that lacks a
scenario is absent from that test's parameters.

Same-seed runs, predict, checkpoint / export and local_run are collected here, parametrised over the table.
The trajectory tests (per model, beside the other options, with dropout, with sample weights), the wrong-size
refusal and the default-sequence test keep their names in tests/test_gpu_<key>.py, beside the option's
kernels and whatever only it has; their bodies are in tests/_side_options.py."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from deep_learning_amd.engine import CTREngine, ModelSpec
from oracle import ctr_ref as R
from tests._side_options import B_, CASES, TOL, _batches, _engine, _init, _run

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _over(pick):
    """parametrize over the Cases that have the scenario `pick` names."""
    cases = [c for c in CASES if getattr(c, pick) is not None]
    return pytest.mark.parametrize("case", cases, ids=[c.key for c in cases])


@_over("same_seed")
def test_same_seed_runs_agree_bit_for_bit(hip_lib, case):
    """Device-initialised engines of one seed, five graph steps each: logits, every parameter and the
    option's moments equal bit for bit; its variables are drawn as the Case's rule says."""
    s = case.same_seed
    bs = _batches(case, s.model, 5, seed=3)
    out = []
    for _ in range(2):
        eng = _engine(case, s.model, s.value, seed=7, adam="lazy")
        p0 = eng.params()
        zs, _ = _run(eng, bs, graph_from=0)
        out.append((zs, eng.params(), eng.dense_state() if s.v_keys else None, p0))
    for a, b in zip(out[0][0], out[1][0]):
        np.testing.assert_array_equal(a, b)
    for k in out[0][1]:
        np.testing.assert_array_equal(out[0][1][k], out[1][1][k], err_msg=k)
    for k in s.v_keys:
        np.testing.assert_array_equal(out[0][2]["v"][k], out[1][2]["v"][k], err_msg=k)
    s.drawn(out[0][3], eng)


@_over("predict")
def test_predict_on_planes_equals_the_record_path(hip_lib, case):
    """Lazy tables: predict right after training, after flush() and after flush(planes=True) (the plane
    lookup, unfused because the option reads x0) give the same bits, and they are the restatement's logits
    within 1e-5."""
    name = "dnn_pipeline"
    if case.predict.seeded:
        eng = _engine(case, name, seed=9, adam="lazy")
    else:
        eng = _engine(case, name, init="none", adam="lazy")
        eng.load_params(_init(case, name, 9)[1])
    bs = _batches(case, name, 6, seed=40)
    for b in bs[:3]:
        eng.train_step(b, graph=True)
    torch.cuda.synchronize()
    if case.predict.gather_rows is not None:
        assert eng.fused_gather_rows() and not eng.fused_gather_l0()
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
    ref = case.forward(R.make_cfg(name, **case.KW[name]), eng.params(), b, case.value)
    assert np.abs(z0 - ref["z"]).max() < TOL


@_over("ckpt")
def test_checkpoint_and_export_round_trip(hip_lib, case, tmp_path):
    """A checkpoint saved after three steps and restored into a fresh model continues the trajectory bit
    for bit (logits of two more steps, every parameter, the option's moments); the exported model loads with
    the option and scores identically."""
    from deep_learning_amd.models._ctr_model import export_model, load_model
    from deep_learning_amd.models.dnn_pipeline import DeepModel
    ck, kw = case.ckpt, case.KW["dnn_pipeline"]
    args = types.SimpleNamespace(epochs=1, batch_size=B_, model_pb=str(tmp_path / "pb"),
                                 save_model_checkpoint=str(tmp_path / "ck"), model_restore=0,
                                 restore_model_checkpoint=str(tmp_path / "ck"), embedding_size=kw["E"],
                                 cate_feats_size=kw["cate_index_size"], hidden_units=kw["hidden"], learning_rate=1e-3,
                                 l2_reg=1e-5, learning_rate_decay_steps=1000, learning_rate_decay_rate=0.9,
                                 cate_field_size=kw["S"], cont_field_size=kw["C"], vector_feats_size=kw["V"],
                                 **ck.args)
    bs = _batches(case, "dnn_pipeline", 5, seed=60)
    a = DeepModel(args, bs)
    a.model_optimizer()
    assert ck.built(a.engine)
    for b in bs[:3]:
        a.engine.train_step(b, graph=True)
    a._save_checkpoint(args.save_model_checkpoint)
    r = DeepModel(args, bs)
    r.model_optimizer()
    r._restore(args.restore_model_checkpoint)
    for m in (a, r):
        m.zs = []
        for b in bs[3:]:
            m.engine.train_step(b, graph=True)
            torch.cuda.synchronize()
            m.zs.append(m.engine.z[:B_].cpu().numpy().copy())
    for x, y in zip(a.zs, r.zs):
        np.testing.assert_array_equal(x, y)
    pa, pr = a.engine.params(), r.engine.params()
    if ck.params:
        ck.params(pa)
    for k in pa:
        np.testing.assert_array_equal(pa[k], pr[k], err_msg=k)
    if ck.moments:
        sa, sr = a.engine.dense_state(), r.engine.dense_state()
        for mv in ("m", "v"):
            for k in ck.moments:
                assert not ck.nonzero or np.abs(sa[mv][k]).max() > 0
                np.testing.assert_array_equal(sa[mv][k], sr[mv][k], err_msg=k)
    export_model(a.engine, args.model_pb)
    loaded = load_model(args.model_pb)
    assert ck.loaded(loaded)
    np.testing.assert_array_equal(loaded.predict(bs[0]), a.engine.predict(bs[0]))


@_over("local")
def test_local_run_train_then_predict(hip_lib, case, tmp_path):
    """local_run.py dnn_pipeline ... <the option's arguments>: train -> export -> predict end to end; the
    exported variables hold the option's and the printed AUC is the restatement's on them within 1e-4."""
    from deep_learning_amd.synthetic import make_batch
    from deep_learning_amd.utils import data_loader
    conf, tr, pr = tmp_path / "conf", tmp_path / "train", tmp_path / "pred"
    for p in (conf, tr, pr):
        p.mkdir()
    lines = ["f%d\tx\tfloat" % i for i in range(13)] + ["c%d\tx\tstring" % i for i in range(26)]
    (conf / "dnn.conf").write_text("\n".join(lines) + "\n")
    V = 3000
    for i in range(3):
        data_loader.write_tfrecord_part(str(tr / ("part-%d" % i)), make_batch(256, cate_index_size=V, seed=i))
    pred_part = make_batch(200, cate_index_size=V, seed=99)
    data_loader.write_tfrecord_part(str(pr / "part-0"), pred_part)
    args = ["dnn_pipeline", "train", "1", "8", str(V), "3", str(conf), str(tr) + "/", str(pr) + "/",
            str(tmp_path / "model_pb"), str(tmp_path / "ckpt"), "0", str(tmp_path / "ckpt"),
            "batch_size=64", "hidden_units=32,16", "shuffle=0"] + case.local.args
    r = subprocess.run([sys.executable, os.path.join(ROOT, "local_run.py")] + args, capture_output=True, text=True,
                       timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert case.local.line is None or case.local.line in r.stdout
    auc_gpu = float(r.stdout.split("val of auc:")[-1].split()[0])
    d = np.load(tmp_path / "model_pb" / "variables.npz")
    P = {k: d[k] for k in d.files}
    case.local.exported(P)
    kw = dict(C=13, V=0, S=26, E=8, cate_index_size=V, hidden=[32, 16])
    b = {k: v[:192] for k, v in pred_part.items()}
    ref = case.forward(R.make_cfg("dnn_pipeline", **kw), P, b, case.local.value, **case.local.ref)
    assert abs(R.auc(b["label"], ref["p"]) - auc_gpu) < 1e-4
