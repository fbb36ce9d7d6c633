"""GPU checks of the dense side-branch parameter groups (deep_learning_amd/param_groups.py, CTREngine.groups
and .bn_groups) with every branch on at once: the groups' order, the checkpoint's key names, a save / restore
through params() + _adam_state that continues bit for bit, and a batch smaller than max_batch (the slab's
capacity against the rows a step fills)."""
import numpy as np
import pytest
import torch

from deep_learning_amd.engine import CTREngine, ModelSpec
from deep_learning_amd.models._ctr_model import _adam_state, _load_adam_state
from tests import _cross_ref as X

pytestmark = pytest.mark.gpu

NAME = "dnn_pipeline"
KW = dict(C=13, V=3, S=8, E=8, cate_index_size=1000, hidden=[32, 16])
B_ = 64
ALL = dict(cross_layers=2, afm_attention=4, ccpm_filters=(2, 2), bi_interaction=True)
COMMON_KEYS = {"adam/opt", "adam/steps", "adam/table_m", "adam/table_v", "adam/hm", "adam/hv", "adam/Wm0", "adam/Wv0",
               "adam/Wm1", "adam/Wv1", "adam/cm", "adam/cv", "adam/am", "adam/av", "adam/km", "adam/kv"}
# tag -> (the options, list(eng.groups), the checkpoint's Adam keys)
CONFIGS = {"pnn": (dict(ALL, pnn="inner"), ["cross", "afm", "ccpm", "pnn"], COMMON_KEYS | {"adam/pm", "adam/pv"}),
           "bn": (dict(ALL, batch_norm=True), ["cross", "afm", "ccpm"],
                  COMMON_KEYS | {"adam/bn_m0", "adam/bn_v0", "adam/bn_m1", "adam/bn_v1"})}


def _engine(opts, max_batch=B_):
    return CTREngine(ModelSpec(NAME, **opts, **KW), max_batch=max_batch, seed=3, adam="lazy")


def _batches(n, seed, B=B_):
    return [X.make_batch(NAME, KW, B, seed + i) for i in range(n)]


def _steps(eng, bs, graph):
    zs = []
    for b in bs:
        eng.train_step(b, graph=graph)
        torch.cuda.synchronize()
        zs.append(eng.z[: eng.last_batch].cpu().numpy().copy())
    eng.check_error()
    return zs


def _assert_same_state(a, b):
    Pa, Pb = a.params(), b.params()
    assert set(Pa) == set(Pb)
    for k in Pa:
        np.testing.assert_array_equal(Pa[k], Pb[k], err_msg=k)
    Da, Db = a.dense_state(), b.dense_state()
    for mv in ("m", "v"):
        assert set(Da[mv]) == set(Db[mv]) and set(Da[mv]) == set(a.dense_params()) - {
            k for k in Pa if k.endswith(("running_mean", "running_var"))}
        for k in Da[mv]:
            np.testing.assert_array_equal(Da[mv][k], Db[mv][k], err_msg="%s %s" % (mv, k))


@pytest.mark.parametrize("tag", list(CONFIGS))
def test_save_restore_continues_bit_for_bit(hip_lib, tmp_path, tag):
    """Three steps, params() + _adam_state into a file, a fresh engine restored from it, two more steps in
    both: the same logits, parameters and moments, bit for bit; the file's Adam keys and the groups' order
    as written out here."""
    opts, names, keys = CONFIGS[tag]
    bs = _batches(5, seed=40)
    eng = _engine(opts)
    assert list(eng.groups) == names and len(eng.bn_groups) == (2 if tag == "bn" else 0)
    _steps(eng, bs[:2], graph=False)
    _steps(eng, bs[2:3], graph=True)
    adam = _adam_state(eng)
    assert set(adam) == keys
    np.savez(tmp_path / "ck.npz", **{"param/" + k: v for k, v in eng.params().items()}, **adam)
    d = np.load(tmp_path / "ck.npz", allow_pickle=False)
    fresh = _engine(opts)
    fresh.load_params({k[len("param/"):]: d[k] for k in d.files if k.startswith("param/")})
    _load_adam_state(fresh, d)
    za, zb = _steps(eng, bs[3:], graph=True), _steps(fresh, bs[3:], graph=True)
    for a, b in zip(za, zb):
        assert np.abs(a).max() > 0
        np.testing.assert_array_equal(a, b)
    _assert_same_state(eng, fresh)
    for g in eng.all_groups():      # every group has trained: no moment is still all zero
        assert np.abs(adam[g.ckpt_keys[0]]).max() > 0 and np.abs(adam[g.ckpt_keys[1]]).max() > 0, g.name


def test_batch_below_max_batch(hip_lib):
    """A batch of 48 in an engine built for 64 (slabs of dl_<x>_grid(64) rows, of which the step fills and
    sums dl_<x>_grid(48)) against an engine built for 48: bit for bit."""
    opts = CONFIGS["pnn"][0]
    bs = _batches(3, seed=50, B=48)
    big, small = _engine(opts, 64), _engine(opts, 48)
    assert any(g.blocks > g.rows(48) for g in big.groups.values())     # the distinction is live at these sizes
    for eng in (big, small):
        eng.zs = _steps(eng, bs[:2], graph=False) + _steps(eng, bs[2:], graph=True)
    for a, b in zip(big.zs, small.zs):
        np.testing.assert_array_equal(a, b)
    _assert_same_state(big, small)
