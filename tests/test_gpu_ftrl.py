"""FTRL-proximal for the wdl wide weights on the GPU: the kernels against the float64 formulas,
training parity against the float64 restatement (tests/_ftrl_ref.py), bit-identity between the
record and the plane paths, persistence, the load-style runner and the untouched default path."""
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from deep_learning_amd import _lib  # noqa: E402
from deep_learning_amd import engine as engine_mod  # noqa: E402
from deep_learning_amd._lib import call, ptr  # noqa: E402
from deep_learning_amd.engine import CTREngine, ModelSpec  # noqa: E402
from oracle import ctr_ref as R  # noqa: E402
from tests import _ftrl_ref as FR  # noqa: E402

TOL = 1e-5                      # the project's f32 parity tolerance
BF16_Z, BF16_LOSS = 3e-2, 5e-3  # the stated bf16-tower tolerance (tests/test_gpu_parity.py)
SCALE = 2.0 ** 48               # DL_WIDE_GRAD_SCALE

# ---------------------------------------------------------------------------------- kernels
ROWS, FW, H = 200, 4, 8
K_LR, K_L1, K_L2 = 0.05, 0.01, 0.1
# f32 kernel against the float64 formulas on the same f32 inputs: the largest term is sigma's
# rounding, 2 ulp of sqrt(n) <= 1 (1.2e-7) / lr (0.05) * |w| (<= 0.4) = 1e-6; z's and w's own
# roundings are below 1e-7
K_TOL = 2e-6
K_SEED = {1: 1, 63: 1, 300: 0}   # chosen on the CPU: the reference's L1 margin exceeds 10 * K_TOL


def _kernel_case(B, seed):
    """Two steps' inputs: wide ids over every row (some in [Fw, Fw + H), some repeated; at
    B = 300 id 150 in every sample: a 300-reference segment, past kWideSegShort = 64), dz and the
    deep-output rows' gradient; and the initial records."""
    rng = np.random.default_rng(seed)
    rec = np.zeros((ROWS, 4), np.float32)
    rec[:, 0] = rng.standard_normal(ROWS) * 0.1
    rec[:, 1] = rng.standard_normal(ROWS) * 0.02
    rec[:, 2] = 0.1 + rng.random(ROWS) * 0.3
    steps = []
    for _ in range(2):
        wide = rng.integers(0, ROWS, size=(B, FW)).astype(np.int64)
        wide[0, 0] = FW + 2                      # an id aliasing a deep-output row, in every case
        if B > 1:
            wide[1, :2] = wide[0, 1]             # an id repeated inside the batch
        if B == 300:
            wide[:, 1] = 150
        dz = (rng.standard_normal(B) * 0.02).astype(np.float32)
        gdeep = (rng.standard_normal(H) * 0.05).astype(np.float32)
        steps.append((wide, dz, gdeep))
    return rec, steps


def _fixed(x):
    return np.rint(np.asarray(x, np.float64) * SCALE).astype(np.int64)


def _kernel_ref(rec, steps):
    """The float64 formulas on the kernels' own inputs (gradients through the int64 fixed point
    and back to f32, as the kernels read them).  Returns (w, z, n, margin, touched)."""
    w, z, n = (rec[:, i].astype(np.float64) for i in range(3))
    margin, ever = np.inf, np.zeros(ROWS, bool)
    for wide, dz, gdeep in steps:
        q = np.zeros(ROWS, np.int64)
        np.add.at(q, wide.reshape(-1), np.repeat(_fixed(dz), FW))
        q[FW:FW + H] += _fixed(gdeep)
        g = (q.astype(np.float64) / SCALE).astype(np.float32).astype(np.float64)
        rows = np.union1d(np.unique(wide), np.arange(FW, FW + H))
        z1 = FR.ftrl_apply(w, z, n, g, rows, K_LR, K_L1, K_L2)
        margin = min(margin, float(np.abs(np.abs(z1) - K_L1).min()))
        ever[rows] = True
    return w, z, n, margin, ever


class _Dev:
    """The buffers of one kernel-level run (the engine's wide_lazy set, by hand)."""

    def __init__(self, rec, B):
        dev = "cuda"
        nw = B * FW
        self.nw = nw
        self.rec = torch.from_numpy(rec.copy()).to(dev)
        self.opt = torch.zeros(_lib.OPT_LEN, device=dev)
        self.wloc = torch.zeros(FW + H + nw + 4, device=dev)
        self.gloc = torch.zeros(FW + H + nw, dtype=torch.int64, device=dev)
        self.stash = torch.zeros(nw, 4, device=dev)
        self.dmark = torch.zeros(16, dtype=torch.uint8, device=dev)
        self.lng = torch.zeros(nw + 1, dtype=torch.int32, device=dev)

    def index(self, wide):
        flat = wide.reshape(-1)
        order = np.argsort(flat, kind="stable")
        uniq, cnt = np.unique(flat, return_counts=True)
        t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).astype(dt)).cuda()
        self.uniq = torch.zeros(self.nw, dtype=torch.int32, device="cuda")
        self.uniq[: uniq.size] = t(uniq, np.int32)
        self.refs = t(order, np.int32)
        self.off = torch.zeros(self.nw + 1, dtype=torch.int32, device="cuda")
        self.off[: uniq.size + 1] = t(np.r_[0, np.cumsum(cnt)], np.int32)
        self.n_uniq = torch.tensor([uniq.size, 0, 0, 0], dtype=torch.int32, device="cuda")
        return uniq

    def gather(self, train=True):
        call("dl_wide_ftrl_gather", ptr(self.rec), ROWS, ptr(self.uniq), ptr(self.n_uniq), self.nw, FW, H,
             ptr(self.opt), ptr(self.wloc), ptr(self.stash) if train else None, _lib.stream_handle())

    def grads(self, dz, gdeep):
        """gloc as the engine's step leaves it before the update: dl_wide_seg_grad's segment sums
        and the deep-output rows' folded batch sums."""
        s = _lib.stream_handle()
        dzt = torch.from_numpy(dz).cuda()
        call("dl_wide_seg_grad", ptr(dzt), FW, ptr(self.refs), ptr(self.off), ptr(self.n_uniq), self.nw, self.nw,
             ptr(self.gloc[FW + H:]), ptr(self.lng), ptr(self.opt), s)
        self.gloc[FW:FW + H] += torch.from_numpy(_fixed(gdeep)).cuda()

    def update(self):
        call("dl_wide_ftrl_update", ptr(self.rec), ptr(self.n_uniq), self.nw, ptr(self.stash), ptr(self.gloc), FW, H,
             K_LR, K_L1, K_L2, ptr(self.opt), ptr(self.dmark), _lib.stream_handle())

    def step(self, wide, dz, gdeep):
        uniq = self.index(wide)
        self.gather()
        self.grads(dz, gdeep)
        self.update()
        torch.cuda.synchronize()
        return uniq


def _run_kernels(B):
    rec, steps = _kernel_case(B, K_SEED[B])
    d = _Dev(rec, B)
    for st in steps:
        d.step(*st)
    assert int(d.opt.view(torch.int32)[_lib.OPT_STATUS].item()) == 0
    assert not d.gloc.any().item() and not d.dmark.any().item()     # the gloc protocol: reset by the update
    return rec, steps, d.rec.cpu().numpy()


@pytest.mark.parametrize("B", [1, 63, 300])
def test_ftrl_kernels_match_float64(hip_lib, B):
    rec, steps, out = _run_kernels(B)
    w, z, n, margin, ever = _kernel_ref(rec, steps)
    assert margin > 10 * K_TOL, margin                  # the fixture: no update sits on the L1 threshold
    if B == 300:
        assert max(np.bincount(steps[0][0].reshape(-1)).max(), 0) >= 300 > 64
    for i, ref in enumerate((w, z, n)):
        err = np.abs(out[:, i].astype(np.float64) - ref).max()
        print("B=%d %s max err %.3g" % (B, "wzn"[i], err))
        assert err < K_TOL, ("wzn"[i], err)
    assert np.array_equal(out[:, 0] == 0, w == 0)       # the exact zeros are the reference's
    if B > 1:
        assert (w[ever] == 0).any() and (w[ever] != 0).any()
    assert np.all(out[:, 3] == 0)
    # untouched rows keep their bits
    assert (~ever).any() or B == 300
    assert np.array_equal(out[~ever].view(np.int32), rec[~ever].view(np.int32))
    # the same inputs give the same bits
    _, _, again = _run_kernels(B)
    assert np.array_equal(out.view(np.int32), again.view(np.int32))


def test_ftrl_gather_forms(hip_lib):
    """wloc = [- | deep rows | unique rows], the stash carries (w, z, n, row bits); a NULL stash
    (the predict form) writes the same wloc and no stash."""
    rec, steps = _kernel_case(63, 5)
    wide = steps[0][0]
    d = _Dev(rec, 63)
    uniq = d.index(wide)
    d.stash.fill_(-7.0)
    d.gather(train=False)
    torch.cuda.synchronize()
    wloc = d.wloc.cpu().numpy()
    assert np.array_equal(wloc[FW:FW + H], rec[FW:FW + H, 0])
    assert np.array_equal(wloc[FW + H:FW + H + uniq.size], rec[uniq, 0])
    assert (d.stash == -7.0).all().item()
    d.gather(train=True)
    torch.cuda.synchronize()
    st = d.stash.cpu().numpy()[: uniq.size]
    assert np.array_equal(st[:, :3], rec[uniq, :3])
    assert np.array_equal(st[:, 3].view(np.int32), uniq.astype(np.int32))
    assert np.array_equal(d.wloc.cpu().numpy(), wloc)


def test_ftrl_poisoned_step_writes_nothing(hip_lib):
    rec, steps = _kernel_case(63, 5)
    d = _Dev(rec, 63)
    d.opt.view(torch.int32)[_lib.OPT_SKIP] = 1
    d.step(*steps[0])
    assert np.array_equal(d.rec.cpu().numpy().view(np.int32), rec.view(np.int32))
    assert not d.gloc.any().item() and not d.dmark.any().item()


def test_ftrl_out_of_range_row_raises_index(hip_lib):
    """A unique row outside [0, w_rows) is never read: DL_STATUS_INDEX, the step poisoned, no
    record written."""
    rec, steps = _kernel_case(63, 5)
    wide, dz, gdeep = steps[0]
    d = _Dev(rec, 63)
    uniq = d.index(wide)
    d.uniq[uniq.size - 1] = ROWS + 5
    d.gather()
    d.grads(dz, gdeep)
    d.update()
    torch.cuda.synchronize()
    st = d.opt.view(torch.int32)
    assert int(st[_lib.OPT_STATUS].item()) & _lib.STATUS_INDEX and int(st[_lib.OPT_SKIP].item()) != 0
    assert np.array_equal(d.rec.cpu().numpy().view(np.int32), rec.view(np.int32))
    assert not d.gloc.any().item() and not d.dmark.any().item()


def test_ftrl_rows_is_the_record_step(hip_lib):
    """dl_ftrl_rows on planes: bit for bit the record kernels' step on the flagged rows, the
    gradient and the flags reset; a row count that is no multiple of 4."""
    rec, steps = _kernel_case(63, 5)
    d = _Dev(rec, 63)
    d.step(*steps[0])
    out = d.rec.cpu().numpy()
    wide, dz, gdeep = steps[0]
    n = ROWS - 1 if not (wide == ROWS - 1).any() else ROWS
    q = np.zeros(ROWS, np.int64)
    np.add.at(q, wide.reshape(-1), np.repeat(_fixed(dz), FW))
    q[FW:FW + H] += _fixed(gdeep)
    touched = np.zeros(ROWS + 8, np.uint8)
    touched[np.union1d(np.unique(wide), np.arange(FW, FW + H))] = 1
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    w, z, nn, g, tch = t(rec[:, 0]), t(rec[:, 1]), t(rec[:, 2]), t(q), t(touched)
    opt = torch.zeros(_lib.OPT_LEN, device="cuda")
    call("dl_ftrl_rows", ptr(w), ptr(z), ptr(nn), ptr(g), ptr(tch), n, K_LR, K_L1, K_L2, ptr(opt), _lib.stream_handle())
    torch.cuda.synchronize()
    for i, a in enumerate((w, z, nn)):
        assert np.array_equal(a.cpu().numpy()[:n].view(np.int32), out[:n, i].view(np.int32)), "wzn"[i]
    assert not g[:n].any().item() and not tch[:n].any().item()


# ---------------------------------------------------------------------------------- training
KW = dict(C=3, S=4, E=8, cate_index_size=50, hidden=[16, 8], Fw=3)
B, STEPS, ID_HI = 64, 5, 40          # wide ids in [0, 40): rows 40..57 are never touched
LR = 0.05
SEED, L1 = 13, 0.015                  # chosen on the CPU: the reference's L1 margin exceeds 1e-4
_REF = {}


def _batches(weight=False):
    return [FR.make_batch(KW, B, seed=SEED * 100 + i, id_hi=ID_HI, weight=weight) for i in range(STEPS)]


def _init():
    cfg = R.make_cfg("wdl", **KW)
    return cfg, R.init_params(cfg, np.random.default_rng(SEED))


def _reference(l1):
    """Five reference steps, computed once: per-step logits and losses, the final state."""
    if l1 not in _REF:
        cfg, P = _init()
        ref = FR.FtrlRef(cfg, P, LR, l1, 0.0)
        fws = [ref.train_step(b) for b in _batches()]
        _REF[l1] = (ref, [f["z"] for f in fws], [f["loss"] for f in fws])
    return _REF[l1]


def _engine(adam, tower="f32", l1=L1, **kw):
    _, P = _init()
    eng = CTREngine(ModelSpec("wdl", tower=tower, wide_optimizer="ftrl", wide_lr=LR, wide_l1=l1, **KW), max_batch=B,
                    init="none", adam=adam, **kw)
    eng.load_params(P)
    return eng


def _state(eng):
    ds = eng.dense_state()
    return (eng.params()["wdl_weights"][:, 0], ds["ftrl/z"][:, 0], ds["ftrl/n"][:, 0])


@pytest.mark.parametrize("l1", [0.0, L1])
@pytest.mark.parametrize("tower", ["f32", "bf16"])
@pytest.mark.parametrize("adam", ["dense", "lazy"])
def test_ftrl_training_matches_restatement(hip_lib, adam, tower, l1):
    ref, zs, losses = _reference(l1)
    if l1 > 0:
        # the L1 threshold is discontinuous: the fixture is valid only with every update's
        # | |z'| - l1 | above ten times the tolerance (no case excluded)
        assert ref.margin > 1e-4, ref.margin
        assert (ref.w[ref.ever] == 0).any() and (ref.w[ref.ever] != 0).any()
    tz, tl, tp = (BF16_Z, BF16_LOSS, BF16_Z) if tower == "bf16" else (TOL, TOL, TOL)
    eng = _engine(adam, tower, l1)
    for i, b in enumerate(_batches()):
        eng.train_step(b)
        ez = np.abs(eng.z[:B].cpu().numpy() - zs[i]).max()
        el = abs(eng.loss() - losses[i])
        print("step %d logit err %.3g loss err %.3g" % (i, ez, el))
        assert ez < tz and el < tl, (i, ez, el)
    eng.check_error()
    w, z, n = _state(eng)
    for name, got, want in (("w", w, ref.w), ("z", z, ref.z), ("n", n, ref.n)):
        err = np.abs(got - want).max()
        print("%s err %.3g" % (name, err))
        assert err < tp, (name, err)
    assert np.array_equal(w == 0, ref.w == 0)
    assert eng.wide_nonzero() == int((ref.w != 0).sum())
    assert np.array_equal(w[~ref.ever], _init()[1]["wdl_weights"][~ref.ever, 0])     # untouched rows: init bits


def _bits(*arrays):
    return [np.ascontiguousarray(a).view(np.int32).copy() for a in arrays]


def _run(adam, weight=False, steps=STEPS, eng=None, start=0, **kw):
    # (the dense table with the sorted backward: its atomic form adds the table's f32 gradients in
    # arrival order, which no bit-identity can rest on — tests/test_gpu_parity.py does the same)
    eng = eng or _engine(adam, sample_weight=weight, **dict({"bwd": "sorted"} if adam == "dense" else {}, **kw))
    zs = []
    for b in _batches(weight)[start:steps]:
        eng.train_step(b)
        zs.append(eng.z[:B].cpu().numpy())
    eng.check_error()
    return eng, _bits(*zs, *_state(eng), eng.params()["weight_mat"], eng.params()["wdl_bias"])


@pytest.mark.parametrize("weight", [False, True])
def test_ftrl_lazy_is_dense_bit_for_bit(hip_lib, weight):
    """Records (dl_wide_ftrl_gather / _update) against planes (dl_ftrl_rows), rows that are both
    wide ids and deep-output rows included; and two same-seed runs of one mode."""
    assert any(np.isin(b["wide_feats"], np.arange(KW["Fw"], KW["Fw"] + 8)).any() for b in _batches())
    _, lazy = _run("lazy", weight)
    _, dense = _run("dense", weight)
    _, again = _run("lazy", weight)
    for a, b_, c in zip(lazy, dense, again):
        assert np.array_equal(a, b_) and np.array_equal(a, c)


def test_ftrl_checkpoint_continues_bit_for_bit(hip_lib, tmp_path):
    from deep_learning_amd.models._ctr_model import _adam_state, _load_adam_state
    _, whole = _run("lazy")
    eng, _ = _run("lazy", steps=3)
    state = {"param/" + k: v for k, v in eng.params().items()}
    state.update(_adam_state(eng))
    assert "ftrl/z" in state and "ftrl/n" in state and "param/ftrl/z" in state
    np.savez(tmp_path / "model-3.npz", **state)
    d = np.load(tmp_path / "model-3.npz", allow_pickle=False)
    P = {k[len("param/"):]: d[k] for k in d.files if k.startswith("param/")}
    new = CTREngine(eng.spec, max_batch=B, init="none", adam="lazy")
    new.load_params(P)
    _load_adam_state(new, d)
    _, rest = _run("lazy", eng=new, start=3)
    for a, b_ in zip(whole[3:], rest):              # steps 3, 4 logits, then the final state
        assert np.array_equal(a, b_)
    # a checkpoint of the other wide optimizer is refused, both ways
    adam_eng = CTREngine(ModelSpec("wdl", **KW), max_batch=B, init="none", adam="lazy")
    with pytest.raises(ValueError, match="wide_optimizer"):
        adam_eng.load_params(P)
    with pytest.raises(ValueError, match="wide_optimizer"):
        _load_adam_state(adam_eng, d)
    adam_eng.load_params(_init()[1])
    astate = _adam_state(adam_eng)
    np.savez(tmp_path / "adam.npz", **astate)
    with pytest.raises(ValueError, match="wide_optimizer"):
        _load_adam_state(new, np.load(tmp_path / "adam.npz", allow_pickle=False))


def test_ftrl_export_load_and_plane_predict(hip_lib, tmp_path, monkeypatch):
    from deep_learning_amd.models._ctr_model import export_model, load_model
    eng, _ = _run("lazy")
    b = _batches()[0]
    want = eng.predict(b)
    export_model(eng, str(tmp_path / "pb"))
    new = load_model(str(tmp_path / "pb"), max_batch=B)
    assert new.ftrl and new.spec.wide_l1 == L1 and new.spec.ftrl_lr == LR
    assert np.array_equal(_bits(new.predict(b))[0], _bits(want)[0])
    for a, b_ in zip(_state(new), _state(eng)):
        assert np.array_equal(_bits(a)[0], _bits(b_)[0])
    assert new.wide_nonzero() == eng.wide_nonzero()
    # predict on the flushed table's planes against the records
    monkeypatch.setenv("DLAMD_FLAT_PLANES", "0")
    recs = load_model(str(tmp_path / "pb"), max_batch=B)
    assert not recs.flat_planes and new.flat_planes
    assert np.array_equal(_bits(recs.predict(b))[0], _bits(want)[0])


def test_ftrl_runner_train_then_predict(hip_lib, tmp_path, capsys):
    """models/wdl.py's DeepModel with local_run's overrides: fit (graph replay, prefetched
    batches) then predict from the exported model; the AUC is the restatement's."""
    from deep_learning_amd.models.wdl import DeepModel
    args = types.SimpleNamespace(hidden_units=KW["hidden"], epochs=1, batch_size=B, learning_rate=0.001,
                                 model_pb=str(tmp_path / "pb"), l2_reg=1e-5, cont_field_size=KW["C"],
                                 cate_field_size=KW["S"], cate_index_size=KW["cate_index_size"],
                                 embedding_size=KW["E"], wide_field_size=KW["Fw"], learning_rate_decay_steps=10000000,
                                 learning_rate_decay_rate=0.9, wide_optimizer="ftrl", wide_lr=LR, wide_l1=L1, wide_l2=0.0)
    m = DeepModel(args)
    eng = m.model_optimizer()
    assert eng.ftrl and eng.wide_lazy
    P = {k: v for k, v in eng.params().items() if not k.startswith("ftrl/")}
    item = lambda b: {"labels": b["label"], "cont_feats": b["cont_feats"], "cate_feats": b["cate_feats"],
                      "wide_feats": b["wide_feats"]}
    train, val = _batches(), [FR.make_batch(KW, B, seed=900 + i, id_hi=ID_HI) for i in range(2)]
    m.fit([item(b) for b in train], [item(b) for b in val])
    auc = m.predict([item(b) for b in val])
    ref = FR.FtrlRef(R.make_cfg("wdl", **KW), P, LR, L1, 0.0)
    for b in train:
        ref.train_step(b)
    want = R.auc(np.concatenate([b["label"] for b in val]), np.concatenate([ref.predict(b) for b in val]))
    print("auc %.6f restatement %.6f" % (auc, want))
    assert abs(auc - want) < 1e-4


# ---------------------------------------------------------------------------------- default path
def _recorded_step(monkeypatch, spec, adam):
    names = []
    real = engine_mod.call

    def rec(name, *a):
        names.append(name)
        return real(name, *a)
    eng = CTREngine(spec, max_batch=B, init="none", adam=adam)
    eng.load_params(_init()[1])
    monkeypatch.setattr(engine_mod, "call", rec)
    eng.train_step(_batches()[0])
    eng.flush()
    eng.loss()
    monkeypatch.setattr(engine_mod, "call", real)
    eng.check_error()
    return eng, names


# one lazy / dense wdl training step, a flush and a loss read as the parent commit queues them
PARENT_LAZY = ["dl_validate_batch", "dl_index_build_pair", "dl_wide_local_ids", "dl_step_begin", "dl_rec_gather",
               "dl_embed_fwd_indexed", "dl_gemm_s3_nt_gather_rows", "dl_gemm_s3_nt_bits", "dl_wide_rec_gather",
               "dl_wdl_head_fwd_bwd", "dl_wide_seg_grad", "dl_gemm_s3_tn", "dl_gemm_s3_nt_bits", "dl_gemm_s3_tn",
               "dl_gemm_s3_nt", "dl_adam_dense_layers", "dl_rec_bwd_adam", "dl_slab_fold_rows", "dl_adam_dense",
               "dl_wide_rec_update", "dl_loss_accumulate", "dl_rec_flush", "dl_wide_rec_flush"]
PARENT_DENSE_WIDE = ["dl_slab_fold_rows", "dl_adam_dense", "dl_adam_rows", "dl_adam_rows"]


def test_adam_default_queues_the_parents_entry_points(hip_lib, monkeypatch):
    """wide_optimizer="adam" (given or defaulted) queues exactly what the parent commit queues and
    allocates nothing FTRL's; "ftrl" swaps only the wide gather / update and drops the flush."""
    for spec in (ModelSpec("wdl", **KW), ModelSpec("wdl", wide_optimizer="adam", wide_lr=0.5, wide_l1=0.1, **KW)):
        eng, names = _recorded_step(monkeypatch, spec, "lazy")
        assert names == PARENT_LAZY, names
        assert not eng.ftrl and eng.wide_flushes
        _, names = _recorded_step(monkeypatch, spec, "dense")
        assert not [n for n in names if "ftrl" in n]
        assert names[-len(PARENT_DENSE_WIDE) - 1:-1] == PARENT_DENSE_WIDE, names
    _, names = _recorded_step(monkeypatch, ModelSpec("wdl", wide_optimizer="ftrl", wide_lr=LR, wide_l1=L1, **KW), "lazy")
    swap = {"dl_wide_rec_gather": "dl_wide_ftrl_gather", "dl_wide_rec_update": "dl_wide_ftrl_update"}
    assert names == [swap.get(n, n) for n in PARENT_LAZY if n != "dl_wide_rec_flush"], names
