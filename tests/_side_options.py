"""The side options' engine-level tests, as data: one Case per option of deep_learning_amd/branches.py's
BRANCHES, in that order, and the helpers and bodies every such test shares.  tests/test_gpu_side_options.py
collects four of the common tests over this table; tests/test_gpu_<key>.py keeps the option's kernels, whatever
only it has, and the other common tests by name, each a call of its body here on the option's row.

Every option is compared against its own float64 restatement (tests/_<key>_ref.py).  The older modules take
(cfg, L, rng) or (cfg, L, A, rng) positionally, the newer ones (cfg, rng, value, **opts); a Case's
init_params / train_step / forward adapt them to the second form, with the other options named as in the
newest modules (L, A, filters, layers, pnn, bn, bi).  Seeds, shapes and scales are each option's own.

A new option adds one Case here, and a file of its own with its kernels' tests and the calls by name."""
import types
from dataclasses import dataclass, field
from typing import Any, Callable

import numpy as np
import pytest
import torch

from deep_learning_amd import _lib
from deep_learning_amd.engine import CTREngine, ModelSpec
from oracle import ctr_ref as R
from tests import _afm_ref as Af
from tests import _autoint_ref as Ai
from tests import _bi_ref as Bi
from tests import _bn_ref as Bn
from tests import _ccpm_ref as Cc
from tests import _cin_ref as Ci
from tests import _cross_ref as X
from tests import _dropout_ref as D
from tests import _pnn_ref as Pn
from tests import _sample_weight_ref as W

TOL = 1e-5          # the engine (tests/test_gpu_parity.py): absolute, on logits, loss and parameters
MODES = {"atomic": dict(bwd="atomic"), "sorted": dict(bwd="sorted"), "lazy": dict(adam="lazy")}
B_ = 64
NS = types.SimpleNamespace


def _s():
    return _lib.stream_handle()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _dnn_kw(hidden):
    return {"dnn_pipeline": dict(C=13, V=3, S=8, E=8, cate_index_size=1000, hidden=hidden),
            "dnn_cate": dict(V=2, S=8, E=8, cate_index_size=1000, hidden=hidden),
            "dnn_multi": dict(C=5, V=2, S=4, E=8, cate_index_size=1000, hidden=hidden,
                              multi_ranges=[[0, 7, "a"], [7, 12, "b"]]),
            "dnn_multi_cate": dict(V=0, S=4, E=8, cate_index_size=1000, hidden=hidden,
                                   multi_ranges=[[0, 5, "a"], [5, 6, "b"]])}


# --------------------------------------------------------------------------- the shared helpers
def _batches(case, name, n, seed=11, B=B_, kw=None):
    return [case.make_batch(name, kw or case.KW[name], B, seed + i) for i in range(n)]


def _init(case, name, seed, value=None, kw=None, **opts):
    """Injected parameters at the models' init scales (the table at the Case's EMB_SCALE, if it has one)."""
    cfg = R.make_cfg(name, **(kw or case.KW[name]))
    rng = np.random.default_rng(seed)
    P = case.init_params(cfg, rng, case.value if value is None else value, **opts)
    if case.EMB_SCALE:
        P["feats_emb"] = (rng.standard_normal(P["feats_emb"].shape) * case.EMB_SCALE).astype(np.float32)
    case.after_init(P)
    return cfg, P


def _ref_steps(case, name, P0, bs, value=None, kw=None, per_step=None, rules=None, **opts):
    """The restatement's steps, watched by the Case's rules (or the ones given): logits, losses, the final
    parameters and the rules' watchers."""
    value = case.value if value is None else value
    cfg = R.make_cfg(name, **(kw or case.KW[name]))
    P = {k: v.copy() for k, v in P0.items()}
    opt = R.AdamTF1(cfg, P)
    watch = [r(value, opts) for r in (case.rules if rules is None else rules)]
    zs, losses = [], []
    for i, b in enumerate(bs):
        for w in watch:
            w.before(P)
        fw = case.train_step(cfg, P, opt, b, value, **opts, **(per_step(i, b) if per_step else {}))
        for w in watch:
            w.after(i, fw)
        zs.append(fw["z"])
        losses.append(fw["loss"])
    return zs, losses, P, watch


def _ref_run(case, name, P0, bs, **kw):
    """_ref_steps, every rule holding: the float32 engine must not be able to decide otherwise than the
    float64 restatement (the seeds are chosen so)."""
    zs, losses, P, watch = _ref_steps(case, name, P0, bs, **kw)
    for w in watch:
        assert w.ok(), w.why()
    return zs, losses, P


def _settled(case, name, seeds, bs, value=None, init={}, **kw):
    """Injected parameters and the restatement's trajectory from them.  seeds an int: that seed, and every
    rule must hold; a range: the first of its seeds at which every rule holds."""
    if isinstance(seeds, int):
        _, P0 = _init(case, name, seeds, value, **init)
        return (P0,) + _ref_run(case, name, P0, bs, value=value, **kw)
    for seed in seeds:
        _, P0 = _init(case, name, seed, value, **init)
        zs, losses, P, watch = _ref_steps(case, name, P0, bs, value=value, **kw)
        if all(w.ok() for w in watch):
            for w in watch:
                w.report(name, seed)
            return P0, zs, losses, P
    raise AssertionError("no seed of %r at which every rule holds" % (seeds,))


class CcpmDecided:
    """CCPM's own rule: no sample of any step may be undecided, or the float32 engine could take another
    branch of a ReLU or a pool than the float64 restatement."""

    def __init__(self, filters):
        self.filters, self.bad = filters, None

    def before(self, P):
        self.prev = {k: P[k].copy() for k in Cc.keys(self.filters)}

    def after(self, i, fw):
        if self.bad is None and Cc.undecided(fw["fields"], self.prev, self.filters, exact_ties_ok=True).any():
            self.bad = i

    def ok(self):
        return self.bad is None

    def why(self):
        return "step %d: an undecided sample" % self.bad

    def report(self, name, seed):
        pass


class AutointMargin:
    """AutoInt's own rule: the smallest |U| the restatement saw lies above 1e-5 of the largest, so that the
    engine decides every ReLU alike."""

    def __init__(self):
        self.lo, self.hi = np.inf, 0.0

    def before(self, P):
        pass

    def after(self, i, fw):
        self.lo, self.hi = min(self.lo, fw["u_min"]), max(self.hi, fw["u_max"])

    def ok(self):
        return self.lo > Ai.MARGIN * self.hi

    def why(self):
        return "min |U| %.3g, max |U| %.3g" % (self.lo, self.hi)

    def report(self, name, seed):
        print("AUTOINT_SEED %s %d: min |U| %.3g, max |U| %.3g" % (name, seed, self.lo, self.hi))


_TRAJECTORIES = {}


def trajectory(case, name):
    """The restatement's five steps from injected parameters, once per option and model."""
    if (case.key, name) not in _TRAJECTORIES:
        bs = _batches(case, name, 5)
        P0, zs, losses, P = _settled(case, name, case.traj_seeds, bs)
        _TRAJECTORIES[case.key, name] = (P0, bs, zs, losses, P)
    return _TRAJECTORIES[case.key, name]


def _engine(case, name, value=None, kw=None, spec={}, **ekw):
    return CTREngine(ModelSpec(name, **case.spec(case.value if value is None else value), **spec,
                               **(kw or case.KW[name])), max_batch=B_, **ekw)


def _run(eng, bs, graph_from=2):
    zs, losses = [], []
    for i, b in enumerate(bs):
        eng.train_step(b, graph=i >= graph_from)
        torch.cuda.synchronize()
        zs.append(eng.z[: eng.last_batch].cpu().numpy().copy())
        losses.append(eng.loss())
    eng.check_error()
    return zs, losses


def _check(case, eng, got_z, got_l, zs, losses, P, tag, value=None):
    err = dict(z=max(np.abs(a - b).max() for a, b in zip(got_z, zs)),
               loss=max(abs(a - b) for a, b in zip(got_l, losses)))
    got = eng.params()
    assert set(got) == set(P), set(got) ^ set(P)
    err.update(case.check(case, eng, got, P, case.value if value is None else value))
    print(*case.tag, tag, "max |engine - restatement|:", {k: float(v) for k, v in err.items()})
    for k, v in err.items():
        assert v < TOL, (k, v)
    return got


def _dropout_steps(case, name, seed, keeps):
    """The masks of the header's words (tests/_dropout_ref.py) after every hidden layer whose keep is not 1;
    the tower input is kept."""
    dims = case.KW[name]["hidden"]
    on = [l > 0 and keeps[l] != 1.0 for l in range(len(dims) + 1)]

    def per_step(i, b):
        return dict(masks=[D.keep_mask(seed, i + 1, l, B_, dims[l - 1], keeps[l]) if on[l] else None
                           for l in range(len(on))],
                    invs=[D.inv_keep(keeps[l]) if on[l] else None for l in range(len(on))])
    return per_step


def follow(case, run):
    """One Run: five steps (two eager, three replayed as a hipGraph) in each of its table modes against the
    restatement from its seeds."""
    name, per_step = run.model, None
    bs = _batches(case, name, 5, seed=run.bseed)
    if run.keeps:
        per_step = _dropout_steps(case, name, run.engine["seed"], run.keeps)
    if run.pos_weight:
        for i, b in enumerate(bs):
            b["weight"] = np.random.default_rng(90 + i).choice(np.float32([0, 0.5, 1, 3]), B_).reshape(B_, 1)
        per_step = lambda i, b: dict(w=W.w_eff_f32(b["weight"], b["label"], run.pos_weight)[0])
    P0, zs, losses, P = _settled(case, name, run.seeds, bs, run.value, run.init, per_step=per_step,
                                 rules=run.rules, **run.ref)
    if run.init_rule:
        run.init_rule(P0)
    for mode in run.modes:
        eng = _engine(case, name, run.value, spec=run.spec, init="none", **MODES[mode], **run.engine)
        eng.load_params({k: v.copy() for k, v in P0.items()})
        gz, gl = _run(eng, bs)
        _check(case, eng, gz, gl, zs, losses, P, run.tag % mode if "%s" in run.tag else run.tag, run.value)


# --------------------------------------------------------------------------- the bodies of the tests that keep
# their names in tests/test_gpu_<key>.py
def trajectory_matches_restatement(case, name):
    """Five steps (two eager, three replayed as a hipGraph) in every table mode: each step's logits and loss
    and the final parameters (the option's variables among them) within 1e-5 of the restatement; lazy and
    sorted + dense bit for bit (where the dense pooled scatter is not atomic: no multi-hot model); the same
    steps without the option end elsewhere, and its variables moved."""
    P0, bs, zs, losses, P = trajectory(case, name)
    res = {}
    for mode, ekw in MODES.items():
        eng = _engine(case, name, init="none", **ekw)
        if case.on_rule:
            case.on_rule(eng)
        eng.load_params({k: v.copy() for k, v in P0.items()})
        gz, gl = _run(eng, bs)
        res[mode] = (gz, _check(case, eng, gz, gl, zs, losses, P, "%s %s" % (name, mode)), eng.dense_state())
    for mv in ("m", "v"):
        for k in case.moment_keys:
            assert np.abs(res["lazy"][2][mv][k]).max() > 0
    if case.bitwise(name):
        for a, b in zip(res["lazy"][0], res["sorted"][0]):
            np.testing.assert_array_equal(a, b)
        for k in res["lazy"][1]:
            np.testing.assert_array_equal(res["lazy"][1][k], res["sorted"][1][k], err_msg=k)
        for mv in ("m", "v"):
            for k in case.bitwise_keys(name):
                np.testing.assert_array_equal(res["lazy"][2][mv][k], res["sorted"][2][mv][k], err_msg=k)
    if case.without:
        plain = CTREngine(ModelSpec(name, **case.KW[name]), max_batch=B_, init="none", adam="lazy")
        plain.load_params(case.without(P0, name))
        plain.train_step(bs[0])
        torch.cuda.synchronize()
        assert np.abs(plain.z[:B_].cpu().numpy() - zs[0]).max() > case.gap * TOL
    case.moved(P0, P)


def with_the(case, other):
    """The option beside the others (tests/_side_options.py says which, and on which model)."""
    for run in case.withs[other]:
        follow(case, run)


def wrong_size_parameters_are_refused(case):
    name = "dnn_cate"
    _, P0 = _init(case, name, 1)
    eng = _engine(case, name, case.wrong.value, init="none", adam="lazy")
    with pytest.raises(ValueError, match=case.wrong.match):
        eng.load_params({k: v.copy() for k, v in P0.items()})


def default_queues_the_kernels_it_queued(case, name, adam, monkeypatch):
    """The option off: a step's and a predict's entry-point sequence equals that of an engine built without
    the argument, and holds none of the new entry points or buffers; with it on, the same sequence plus the
    new launches."""
    from deep_learning_amd import engine as E
    names = []
    real = E.call
    monkeypatch.setattr(E, "call", lambda n, *a: (names.append(n), real(n, *a))[1])
    bs = _batches(case, name, 2, seed=70)
    on = case.spec(case.value)
    seqs, seen = [], []
    for extra in ({}, case.off, on):
        eng = CTREngine(ModelSpec(name, **extra, **case.KW[name]), max_batch=B_, seed=3, adam=adam)
        del names[:]
        eng.train_step(bs[0])
        eng.predict(bs[1])
        torch.cuda.synchronize()
        seqs.append(list(names))
        seen.append(case.probe(eng, extra is on))
    assert seqs[0] == seqs[1] and len(seqs[0]) > 8
    assert not any(s in n for n in seqs[0] for s in case.absent)
    case.added(case, seqs, seen, adam)


# --------------------------------------------------------------------------- the rows' parts
@dataclass
class Run:
    """A trajectory scenario."""
    model: str
    seeds: Any                      # the parameter seed, or the range searched for one at which every rule holds
    bseed: int                      # the batch seed
    tag: str                        # printed; "%s" takes the table mode
    value: Any = None               # the option's value, the Case's if None
    init: dict = field(default_factory=dict)        # the restatement's init_params options
    ref: dict = field(default_factory=dict)         # the restatement's train_step options
    spec: dict = field(default_factory=dict)        # further ModelSpec arguments
    engine: dict = field(default_factory=dict)      # further CTREngine arguments
    modes: tuple = ("lazy",)
    rules: Any = None               # in place of the Case's
    init_rule: Callable = None      # an assertion on the injected parameters
    keeps: list = None              # dropout_keep_deep, the masks fed to the restatement
    pos_weight: float = None        # sample weights drawn, the restatement's loss weighted


def _nothing(*a):
    pass


@dataclass
class SameSeed:
    model: str
    value: Any
    drawn: Callable                 # (p0, eng): how the device drew the option's variables
    v_keys: list = None             # whose second moments are compared; None: the option's variables


@dataclass
class Ckpt:
    args: dict                      # the model's further arguments
    built: Callable                 # (engine): the model built the option
    loaded: Callable                # (engine): the exported model loaded with it
    moments: list = None            # whose moments are compared; None: the option's variables
    nonzero: bool = False           # ... and must have moved
    params: Callable = None         # an assertion on the saved model's parameters


@dataclass
class Case:
    """One side option's row.  What a row leaves out is the default written here."""
    key: str
    value: Any                      # the default test value of the spec keyword(s)
    spec: Callable                  # value -> ModelSpec keywords
    keys: Callable                  # value -> the option's variables
    KW: dict                        # model -> its ModelSpec arguments
    init_params: Callable           # (cfg, rng, value, **opts): the restatement's own, adapted
    train_step: Callable            # (cfg, P, opt, b, value, **opts)
    forward: Callable               # (cfg, P, b, value[, **opts])
    check: Callable                 # _check's errors beyond z and loss
    withs: dict                     # scenario name -> [Run]: the option beside the others
    weighted: Run
    same_seed: SameSeed
    ckpt: Ckpt
    local: Any                      # local_run's arguments, stdout line, exported shapes, the forward's value / options
    off: dict                       # ModelSpec keywords of the option switched off
    absent: list                    # substrings no entry point of the default sequence may hold
    probe: Callable                 # (eng, on): the buffers an engine without the option lacks
    added: Callable                 # (case, seqs, seen, adam): the sequence with the option against the default one
    make_batch: Callable = X.make_batch
    EMB_SCALE: float = None         # the injected table's scale
    after_init: Callable = _nothing
    rules: tuple = ()               # (value, opts) -> watcher of the restatement's steps
    tag: tuple = ()                 # printed before _check's line
    traj_seeds: Any = 42
    on_rule: Callable = None        # (eng): asserted of every trajectory engine
    without: Callable = None        # (P0, name) -> the plain engine's parameters; None: no plain engine
    gap: float = None               # ... whose first logits differ by more than gap * TOL
    moved: Callable = _nothing      # (P0, P): the option's variables moved away from the start
    dropout: Run = None
    wrong: Any = None               # the wrong-size value and the refusal's text
    predict: Any = None
    new: list = None                # a chain member's entry points
    moment_keys: list = None        # moments that must be non-zero after the lazy run; None: the option's variables
    bitwise: Callable = None        # name -> lazy equals sorted + dense bit for bit; None: no multi-hot model
    bitwise_keys: Callable = None   # name -> moments compared then; None: the option's variables
    defaults: tuple = (("dnn_pipeline", "dense"), ("dnn_pipeline", "lazy"))     # the default-sequence test's cases

    def __post_init__(self):
        own = self.keys(self.value)
        if self.moment_keys is None:
            self.moment_keys = own
        if self.bitwise is None:
            self.bitwise = lambda name: "multi_ranges" not in self.KW[name]
        if self.bitwise_keys is None:
            self.bitwise_keys = lambda name: own
        if self.same_seed.v_keys is None:
            self.same_seed.v_keys = self.keys(self.same_seed.value)
        if self.ckpt.moments is None:
            self.ckpt.moments = own


def _dropout(seeds, keeps):
    """dnn_cate with dropout_keep_deep = keeps: five lazy steps against the restatement fed the masks."""
    return Run("dnn_cate", seeds, 21, "dropout", keeps=keeps, spec=dict(dropout_keep_deep=keeps), engine=dict(seed=77))


def _weighted(seeds, model="dnn_pipeline"):
    """sample_weight=True and pos_weight 2.5 (weights in {0, 0.5, 1, 3}): five lazy steps against the
    restatement's weighted loss."""
    return Run(model, seeds, 31, "weighted", pos_weight=2.5, spec=dict(pos_weight=2.5), engine=dict(sample_weight=True))


HIDDEN, LATER = [1.0, 0.8, 0.7], [1.0, 1.0, 0.7]      # dropout after both hidden layers, after the second only


def _keys_check(label=None):
    """The option's variables have the restatement's shapes; every parameter, and the option's own under
    `label`, against the restatement."""
    def check(case, eng, got, P, value):
        err = dict(params=max(np.abs(got[k] - P[k]).max() for k in P))
        if label:
            for k in case.keys(value):
                assert got[k].shape == P[k].shape, k
            err[label] = max(np.abs(got[k] - P[k]).max() for k in case.keys(value))
        return err
    return check


def _bi_check(case, eng, got, P, value):
    assert got["deep_0"].shape == P["deep_0"].shape == (eng.spec.deep_in, eng.spec.hidden[0])
    E = eng.spec.E
    return dict(params=max(np.abs(got[k] - P[k]).max() for k in P),
                deep_0_q_rows=np.abs(got["deep_0"][-E:] - P["deep_0"][-E:]).max())


def _bn_check(case, eng, got, P, value):
    bn = [k for k in P if k.startswith("batch_norm")]
    assert len(bn) == 4 * len(eng.spec.hidden) and all(got[k].shape == P[k].shape for k in bn)
    return dict(params=max(np.abs(got[k] - P[k]).max() for k in P if k not in bn),
                biases=max(np.abs(got[k] - P[k]).max() for k in P if k.startswith("deep_bias_")),
                gamma_beta=max(np.abs(got[k] - P[k]).max() for k in bn if not "running" in k),
                running=max(np.abs(got[k] - P[k]).max() for k in bn if "running" in k))


def _without_prefix(prefix):
    return lambda P0, name: {k: v.copy() for k, v in P0.items() if not k.startswith(prefix)}


def _moved(pick, keys):
    """The "ends elsewhere" assertion on the option's own variables: the largest (max) or every (min) of
    them moved away from the start."""
    def moved(P0, P):
        assert pick(np.abs(P[k] - P0[k]).max() for k in keys) > 100 * TOL
    return moved


def _chain_added(case, seqs, seen, adam):
    """A member of the logit chain: the same sequence plus the step's four launches and predict's two, the
    head's entry point exchanged for the one that takes the chain's logit."""
    rest = list(seqs[2])
    for n in case.new + case.new[:2]:
        rest.remove(n)
    assert rest == [n for n in seqs[0] if n != "dl_head_fwd_bwd"]
    assert seqs[0].count("dl_head_fwd_bwd") == 2


def _removed(names):
    def added(case, seqs, seen, adam):
        rest = list(seqs[2])
        for n in names:
            rest.remove(n)
        assert rest == seqs[0]
    return added


def _glorot_within(p0, k, shp):
    lim = np.sqrt(6.0 / (shp[0] + shp[1]))
    assert 0.5 * lim < np.abs(p0[k]).max() <= lim * (1 + 1e-6), (k, np.abs(p0[k]).max(), lim)


# ---- cross
LC = 2


def _cross_drawn(p0, eng):
    """The cross vectors are drawn at their reference scales."""
    Dn, H = eng.D0, CROSS.KW["dnn_multi"]["hidden"][-1]
    for k in X.cross_keys(LC):
        want = np.sqrt(2.0 / (Dn + H + 1)) if k == "cross_res" else np.sqrt(1.0 / Dn)
        assert p0[k].shape == (Dn, 1) and 0.6 * want < p0[k].std() < 1.5 * want, (k, p0[k].std(), want)


def _cross_probe(eng, on):
    assert on or ("cross" not in eng.groups and not any(hasattr(eng, a) for a in ("z_cross", "cross_s")))


def _cross_exported(P):
    assert set(X.cross_keys(2)) <= set(P) and P["cross_res"].shape == (13 + 26 * 8, 1)


CROSS = Case(
    key="cross", value=LC, spec=lambda v: {"cross_layers": v}, keys=X.cross_keys, KW=_dnn_kw([32, 16]),
    init_params=lambda cfg, rng, v: X.init_params(cfg, v, rng),
    train_step=lambda cfg, P, opt, b, v, **o: X.train_step(cfg, P, opt, b, v, **o),
    forward=lambda cfg, P, b, v: X.forward_backward(cfg, P, b, v),
    check=_keys_check(), without=_without_prefix("cross_"), gap=100,
    withs={}, dropout=_dropout(4, HIDDEN), weighted=_weighted(6),
    same_seed=SameSeed(model="dnn_multi", value=LC, drawn=_cross_drawn),
    predict=NS(seeded=True, gather_rows=True),
    ckpt=Ckpt(args=dict(cross_layers=LC), built=lambda e: e.cross == LC,
              loaded=lambda m: m.spec.cross_layers == LC and m.cross == LC),
    local=NS(args=["cross_layers=2"], line="cross_layers = 2", exported=_cross_exported, value=2, ref={}),
    off={"cross_layers": 0}, absent=["cross"], probe=_cross_probe, added=_chain_added,
    new=["dl_cross_fwd", "dl_head_fwd_bwd_cross", "dl_cross_bwd", "dl_adam_dense"])

# ---- afm
AT = 4


def _afm_after_init(P):
    assert np.abs(P["attention_b"]).min() > 1e-3          # u ~ b at this scale: no kink within rounding


def _afm_drawn(p0, eng):
    """The attention variables are drawn at their reference scales and shapes."""
    E = AFM.KW["dnn_multi"]["E"]
    shapes = dict(attention_w=(E, 16), attention_b=(1, 16), attention_h=(1, 16), attention_p=(E, 1))
    for k, shp in shapes.items():
        want = np.sqrt(2.0 / (16 + E)) if k in ("attention_w", "attention_b") else 1.0
        assert p0[k].shape == shp and 0.5 * want < p0[k].std() < 1.7 * want, (k, p0[k].std(), want)


def _afm_probe(eng, on):
    assert on or ("afm" not in eng.groups and not any(hasattr(eng, a) for a in ("z_afm", "afm_stats")))


def _afm_exported(P):
    assert set(Af.AFM_KEYS) <= set(P) and P["attention_w"].shape == (8, 4) and P["attention_p"].shape == (8, 1)


AFM = Case(
    key="afm", value=AT, spec=lambda v: {"afm_attention": v}, keys=lambda v: Af.AFM_KEYS, KW=_dnn_kw([32, 16]),
    after_init=_afm_after_init,
    init_params=lambda cfg, rng, v, L=0: Af.init_params(cfg, L, AT, rng),
    train_step=lambda cfg, P, opt, b, v, L=0, **o: Af.train_step(cfg, P, opt, b, L, AT, **o),
    forward=lambda cfg, P, b, v: Af.forward_backward(cfg, P, b, 0, v),
    check=_keys_check("attention"), gap=5,     # (z_afm ~ 1e-4 at the init scale)
    without=lambda P0, name: {k: v.copy() for k, v in P0.items() if k not in Af.AFM_KEYS},
    moved=_moved(max, Af.AFM_KEYS),
    # dnn_multi with cross_layers = 2 as well: z_cross rides in through z_add
    withs={"the_cross_network": [Run("dnn_multi", 43, 15, "cross + afm", init=dict(L=2), ref=dict(L=2),
                                     spec=dict(cross_layers=2))]},
    dropout=_dropout(4, HIDDEN), weighted=_weighted(6),
    same_seed=SameSeed(model="dnn_multi", value=16, drawn=_afm_drawn),
    predict=NS(seeded=True, gather_rows=True),
    ckpt=Ckpt(args=dict(afm_attention=AT), built=lambda e: e.afm == AT,
              loaded=lambda m: m.spec.afm_attention == AT and m.afm == AT),
    local=NS(args=["afm_attention=4"], line="afm_attention = 4", exported=_afm_exported, value=4, ref={}),
    off={"afm_attention": 0}, absent=["afm", "cross"], probe=_afm_probe, added=_chain_added,
    new=["dl_afm_fwd", "dl_head_fwd_bwd_cross", "dl_afm_bwd", "dl_adam_dense"])

# ---- the three newer chain members: (cfg, rng, value, **opts), the table at EMB_SCALE = 0.3 (z ~ 0.1)
_BI_BN = dict(init=dict(bn=True, bi=True, jitter=0.2), ref=dict(bn=True, bi=True),
              spec=dict(bi_interaction=True, batch_norm=True), modes=("atomic", "lazy"))
_CHAIN = dict(cross_layers=2, afm_attention=4)
FL = (2, 2)


def _ccpm_drawn(p0, eng):
    """The CCPM variables are drawn as Keras does (glorot_uniform kernels within their limit, zero biases)
    in the reference's shapes."""
    for k, shp in Cc.shapes(6, 8, (4, 2)).items():
        assert p0[k].shape == shp, k
        if k.endswith("bias"):
            assert (p0[k] == 0).all()
        else:
            rf = 9 if len(shp) == 4 else 1
            lim = np.sqrt(6.0 / (rf * (shp[-2] + shp[-1])))
            assert 0.5 * lim < np.abs(p0[k]).max() <= lim * (1 + 1e-6), (k, np.abs(p0[k]).max(), lim)


def _ccpm_probe(eng, on):
    assert on or ("ccpm" not in eng.groups and not hasattr(eng, "z_ccpm"))


def _ccpm_exported(P):
    assert set(Cc.keys(FL)) <= set(P)
    assert P["ccpm_conv_1.kernel"].shape == (3, 3, 2, 2) and P["ccpm_out.kernel"].shape == (2 * 6 * 2, 1)


CCPM = Case(
    key="ccpm", value=FL, spec=lambda v: {"ccpm_filters": v}, keys=Cc.keys, KW=_dnn_kw([16, 16]),
    EMB_SCALE=0.3,
    rules=(lambda v, o: CcpmDecided(v),),
    init_params=Cc.init_params, train_step=Cc.train_step, forward=Cc.forward_backward,
    check=_keys_check("ccpm"), without=_without_prefix("ccpm_"), gap=100,
    moved=_moved(max, Cc.keys(FL)),
    withs={
        # dnn_multi with cross_layers = 2 and afm_attention = 4 as well: one logit carries cross, AFM and CCPM,
        # in that order; and with cross_layers alone (z_cross straight into dl_ccpm_fwd)
        "the_cross_network_and_the_attention": [
            Run("dnn_multi", 50, 15, "cross + afm + ccpm", init=dict(L=2, A=4), ref=dict(L=2, A=4), spec=_CHAIN),
            Run("dnn_multi", 44, 15, "cross + ccpm", init=dict(L=2), ref=dict(L=2),
                spec=dict(cross_layers=2, afm_attention=0))],
        # dnn_pipeline with bi_interaction + batch_norm (NFM's tower) beside the branch, lazy and atomic
        "the_pooling_and_batch_norm": [Run("dnn_pipeline", 45, 13, "bi + bn %s", **_BI_BN)],
        # dnn_multi_cate with pnn='inner' as well, and two layers down to a 2 x 1 map (6 fields -> 3 -> 1)
        "the_product_layer": [Run("dnn_multi_cate", 46, 19, "pnn + ccpm", value=(2, 3),
                                  init=dict(pnn=True, theta_scale=0.3), ref=dict(pnn=True), spec=dict(pnn="inner"))]},
    dropout=_dropout(4, HIDDEN), weighted=_weighted(8),
    same_seed=SameSeed(model="dnn_multi", value=(4, 2), drawn=_ccpm_drawn),
    wrong=NS(value=(2, 3), match="ccpm_filters: ccpm_out.kernel holds 8 values, not 12 x 1"),
    predict=NS(seeded=True, gather_rows=True),
    ckpt=Ckpt(args=dict(ccpm_filters=list(FL)), built=lambda e: e.ccpm == FL,
              loaded=lambda m: m.spec.ccpm_filters == FL and m.ccpm == FL),
    local=NS(args=["ccpm_filters=2,2"], line="ccpm_filters = [2, 2]", exported=_ccpm_exported, value=FL, ref={}),
    off={"ccpm_filters": ()}, absent=["ccpm", "afm", "cross"], probe=_ccpm_probe, added=_chain_added,
    new=["dl_ccpm_fwd", "dl_head_fwd_bwd_cross", "dl_ccpm_bwd", "dl_adam_dense"])

CL = (4, 3)


def _cin_drawn(p0, eng):
    """The layers are drawn glorot-uniform within their limit, in the variables' shapes."""
    cl = (8, 4)
    for k, shp in Ci.shapes(6, cl).items():
        assert p0[k].shape == shp, k
        if k == "cin_res":
            assert 0 < np.abs(p0[k]).max() < 6 * np.sqrt(2.0 / (sum(cl) + 1))
        else:
            _glorot_within(p0, k, shp)


def _cin_probe(eng, on):
    assert on or ("cin" not in eng.groups and not hasattr(eng, "z_cin"))


def _cin_exported(P):
    assert set(Ci.keys(CL)) <= set(P)
    assert P["cin_layer_0"].shape == (26 * 26, 4) and P["cin_layer_1"].shape == (4 * 26, 3) and P["cin_res"].shape == (7, 1)


_FOREIGN_CCPM = lambda v, o: CcpmDecided(o["filters"])      # CCPM's rule where it is one of the other options

CIN = Case(
    key="cin", value=CL, spec=lambda v: {"cin_layers": v}, keys=Ci.keys, KW=_dnn_kw([16, 16]),
    EMB_SCALE=0.3,
    init_params=Ci.init_params, train_step=Ci.train_step, forward=Ci.forward_backward,
    check=_keys_check("cin"), without=_without_prefix("cin_"), gap=100,
    moved=_moved(min, Ci.keys(CL)),
    withs={
        # dnn_multi with cross_layers = 2, afm_attention = 4 and ccpm_filters = (2, 2) as well: one logit carries
        # cross, AFM, CCPM and CIN, in that order; CCPM's decisions must be decided in every step (its own rule)
        "the_whole_logit_chain": [Run("dnn_multi", range(50, 70), 15, "cross + afm + ccpm + cin",
                                      init=dict(L=2, A=4, filters=(2, 2)), ref=dict(L=2, A=4, filters=(2, 2)),
                                      spec=dict(ccpm_filters=(2, 2), **_CHAIN), rules=(_FOREIGN_CCPM,))],
        "the_pooling_and_batch_norm": [Run("dnn_pipeline", 45, 13, "bi + bn %s", **_BI_BN)],
        # dnn_multi_cate with pnn='inner' as well, and three layers
        "the_product_layer": [Run("dnn_multi_cate", 46, 19, "pnn + cin", value=(3, 1, 2),
                                  init=dict(pnn=True, theta_scale=0.3), ref=dict(pnn=True), spec=dict(pnn="inner"))]},
    dropout=_dropout(4, HIDDEN), weighted=_weighted(8),
    same_seed=SameSeed(model="dnn_multi", value=(8, 4), drawn=_cin_drawn),
    wrong=NS(value=(4, 5), match="cin_layers: cin_res holds 7 values, not 9 x 1"),
    predict=NS(seeded=True, gather_rows=True),
    ckpt=Ckpt(args=dict(cin_layers=list(CL)), built=lambda e: e.cin == CL,
              loaded=lambda m: m.spec.cin_layers == CL and m.cin == CL),
    local=NS(args=["cin_layers=4,3"], line="cin_layers = [4, 3]", exported=_cin_exported, value=CL, ref={}),
    off={"cin_layers": ()}, absent=["cin", "ccpm", "afm", "cross"], probe=_cin_probe, added=_chain_added,
    new=["dl_cin_fwd", "dl_head_fwd_bwd_cross", "dl_cin_bwd", "dl_adam_dense"])

AI = (2, 2, 8)      # autoint_layers, autoint_heads, autoint_dim
_AUTOINT_RULE = lambda v, o: AutointMargin()
_from = lambda seed0: range(seed0, seed0 + 60)      # the first seed from seed0 on that keeps |U| above the margin


def _autoint_drawn(p0, eng):
    """The matrices are drawn glorot-uniform within their limit, in the variables' shapes."""
    for k, shp in Ai.shapes(6, 8, 2, 16).items():
        assert p0[k].shape == shp, k
        if k == "autoint_res":
            assert 0 < np.abs(p0[k]).max() < 6 * np.sqrt(2.0 / (6 * 16 + 1))
        else:
            _glorot_within(p0, k, shp)


def _autoint_probe(eng, on):
    assert on or ("autoint" not in eng.groups and not hasattr(eng, "z_autoint") and not eng.autoint)


def _autoint_exported(P):
    assert set(Ai.keys(2)) <= set(P)
    assert P["autoint_q_0"].shape == (8, 8) and P["autoint_r_1"].shape == (8, 8) and P["autoint_res"].shape == (26 * 8, 1)


def _autoint_loaded(m):
    sp = m.spec
    return (sp.autoint_layers, sp.autoint_heads, sp.autoint_dim) == AI and m.autoint == 2


AUTOINT = Case(
    key="autoint", value=AI, spec=lambda v: dict(autoint_layers=v[0], autoint_heads=v[1], autoint_dim=v[2]),
    keys=lambda v: Ai.keys(v[0]), KW=_dnn_kw([16, 16]),
    EMB_SCALE=0.3, rules=(_AUTOINT_RULE,), tag=("AUTOINT_ENGINE",),
    init_params=Ai.init_params, train_step=Ai.train_step, forward=Ai.forward_backward,
    check=_keys_check("autoint"), traj_seeds=_from(42), without=_without_prefix("autoint_"), gap=100,
    moved=_moved(min, Ai.keys(AI[0])),
    withs={
        # dnn_multi with cross_layers = 2, afm_attention = 4, ccpm_filters = (2, 2) and cin_layers = (4, 3) as
        # well: one logit carries cross, AFM, CCPM, CIN and AutoInt, in that order
        "the_whole_logit_chain": [Run("dnn_multi", range(50, 70), 15, "cross + afm + ccpm + cin + autoint",
                                      init=dict(L=2, A=4, filters=(2, 2), layers=(4, 3)),
                                      ref=dict(L=2, A=4, filters=(2, 2), layers=(4, 3)),
                                      spec=dict(cin_layers=(4, 3), ccpm_filters=(2, 2), **_CHAIN),
                                      rules=(_FOREIGN_CCPM, _AUTOINT_RULE))],
        "the_pooling_and_batch_norm": [Run("dnn_pipeline", _from(45), 13, "bi + bn %s", **_BI_BN)],
        # dnn_multi_cate with pnn='inner' as well, three layers of four heads
        "the_product_layer": [Run("dnn_multi_cate", _from(46), 19, "pnn + autoint", value=(3, 4, 8),
                                  init=dict(pnn=True, theta_scale=0.3), ref=dict(pnn=True), spec=dict(pnn="inner"))]},
    dropout=_dropout(_from(4), HIDDEN), weighted=_weighted(_from(8)),
    same_seed=SameSeed(model="dnn_multi", value=(2, 4, 16), drawn=_autoint_drawn),
    wrong=NS(value=(2, 2, 16), match="autoint_layers: autoint_res holds 64 values, not 128 x 1"),
    predict=NS(seeded=True, gather_rows=True),
    ckpt=Ckpt(args=dict(autoint_layers=2, autoint_heads=2, autoint_dim=8), built=lambda e: e.autoint == 2,
              loaded=_autoint_loaded),
    local=NS(args=["autoint_layers=2", "autoint_heads=2", "autoint_dim=8"], line="autoint_layers = 2",
             exported=_autoint_exported, value=AI, ref={}),
    off=dict(autoint_layers=0, autoint_heads=4, autoint_dim=32), absent=["autoint", "cin", "ccpm", "afm", "cross"],
    probe=_autoint_probe, added=_chain_added,
    new=["dl_autoint_fwd", "dl_head_fwd_bwd_cross", "dl_autoint_bwd", "dl_adam_dense"])

# ---- pnn
THETA_SCALE = 0.3   # injected theta: lp ~ 1e-2, so the layer moves the logits far beyond the tolerance


def _pnn_drawn(p0, eng):
    """theta is drawn at the reference's scale and shape."""
    th = p0[Pn.KEY]
    assert th.shape == (32, 6) and 0.005 < th.std() < 0.017


def _pnn_probe(eng, on):
    assert on or "pnn" not in eng.groups


def _pnn_exported(P):
    assert P[Pn.KEY].shape == (32, 26)


PNN = Case(
    key="pnn", value="inner", spec=lambda v: {"pnn": v}, keys=lambda v: [Pn.KEY], KW=_dnn_kw([32, 16]),
    init_params=lambda cfg, rng, v, L=0, A=0: Pn.init_params(cfg, L, A, True, rng, scale=THETA_SCALE),
    train_step=lambda cfg, P, opt, b, v, L=0, A=0, **o: Pn.train_step(cfg, P, opt, b, L, A, True, **o),
    forward=lambda cfg, P, b, v: Pn.forward_backward(cfg, P, b, pnn=True),
    check=_keys_check("theta"), gap=5,
    without=lambda P0, name: {k: v.copy() for k, v in P0.items() if k != Pn.KEY},
    moved=_moved(max, [Pn.KEY]),
    # dnn_multi with cross_layers = 2 and afm_attention = 4 as well
    withs={"the_cross_network_and_the_attention": [Run("dnn_multi", 43, 15, "cross + afm + pnn", init=dict(L=2, A=4),
                                                       ref=dict(L=2, A=4), spec=dict(afm_attention=4, cross_layers=2))]},
    dropout=_dropout(4, LATER), weighted=_weighted(6),
    same_seed=SameSeed(model="dnn_multi", value="inner", drawn=_pnn_drawn),
    predict=NS(seeded=False, gather_rows=True),
    ckpt=Ckpt(args=dict(pnn="inner"), built=lambda e: e.pnn == "inner", nonzero=True, moments=[Pn.KEY],
              loaded=lambda m: m.spec.pnn == "inner" and m.pnn == "inner"),
    local=NS(args=["pnn=inner"], line=None, exported=_pnn_exported, value="inner", ref={}),
    off={"pnn": None}, absent=["pnn"], probe=_pnn_probe,
    # the step's three, predict's one
    added=_removed(["dl_pnn_inner_fwd", "dl_pnn_inner_bwd", "dl_adam_dense", "dl_pnn_inner_fwd"]))


# ---- bi
def _bi_on(eng):
    assert eng.bi and not eng.fused_gather_rows() and not eng.fused_gather_l0()


def _bi_moved(P0, P):
    """The pooling's rows of deep_0 train."""
    assert np.abs(P["deep_0"][-8:] - P0["deep_0"][-8:]).max() > 100 * TOL


def _bi_drawn(p0, eng):
    """deep_0 is drawn at the new fan-in."""
    w0 = p0["deep_0"]
    D0 = 6 * 8 + 5 + 2 + 8
    assert w0.shape == (D0, 32) and 0.7 < w0.std() / np.sqrt(2.0 / (D0 + 32)) < 1.3 and np.abs(w0[-8:]).min() > 0


def _bi_probe(eng, on):
    return tuple(eng.x0.shape), tuple(eng.dx0.shape), tuple(eng.W[0].shape), eng.cont_col, eng.dx_cols


def _bi_added(case, seqs, shapes, adam):
    """x0 / dx0 / deep_0 keep their widths with the option off; with it on the lazy step loses the first
    layer's fused row gather and both gain the two launches (predict one)."""
    assert shapes[0] == shapes[1]
    assert shapes[2][3] == shapes[0][3] + 8 and shapes[2][4] == shapes[0][4] + 8
    rest = list(seqs[2])
    for n in ["dl_bi_fwd", "dl_bi_bwd", "dl_bi_fwd"]:   # the step's two, predict's one
        rest.remove(n)
    want = ["dl_gemm_s3_nt_bits" if n == "dl_gemm_s3_nt_gather_rows" else n for n in seqs[0]]
    assert rest == want
    assert ("dl_gemm_s3_nt_gather_rows" in seqs[0]) == (adam == "lazy")


def _bi_cross_is_wider(P0):
    """The cross network is built on the wider input, q included."""
    assert P0["cross_res"].shape[0] == Bi.deep_in(R.make_cfg("dnn_multi", **_dnn_kw([32, 16])["dnn_multi"]), True)


def _bi_exported(P):
    assert P["deep_0"].shape == (13 + 26 * 8 + 8, 32)


BI = Case(
    key="bi", value=True, spec=lambda v: {"bi_interaction": v}, keys=lambda v: [], KW=_dnn_kw([32, 16]),
    EMB_SCALE=0.3,
    init_params=lambda cfg, rng, v, **o: Bi.init_params(cfg, rng, bi=True, theta_scale=0.3, **o),
    train_step=lambda cfg, P, opt, b, v, **o: Bi.train_step(cfg, P, opt, b, bi=True, **o),
    forward=lambda cfg, P, b, v, **o: Bi.forward_backward(cfg, P, b, bi=True, **o),
    check=_bi_check, on_rule=_bi_on, gap=5,
    without=lambda P0, name: dict({k: v.copy() for k, v in P0.items()}, deep_0=P0["deep_0"][:-8].copy()),
    moved=_bi_moved,
    withs={
        # dnn_multi with cross_layers = 2 (on the wider input, q included) and afm_attention = 4 as well
        "the_cross_network_and_the_attention": [Run("dnn_multi", 43, 15, "cross + afm + bi", init=dict(L=2, A=4),
                                                    ref=dict(L=2, A=4), spec=dict(afm_attention=4, cross_layers=2),
                                                    init_rule=_bi_cross_is_wider)],
        "the_product_layer": [Run("dnn_multi_cate", 46, 19, "pnn + bi", init=dict(pnn=True), ref=dict(pnn=True),
                                  spec=dict(pnn="inner"))]},
    dropout=_dropout(4, LATER), weighted=_weighted(6),
    same_seed=SameSeed(model="dnn_multi", value=True, drawn=_bi_drawn),
    predict=NS(seeded=False, gather_rows=None),
    ckpt=Ckpt(args=dict(bi_interaction=True), built=lambda e: e.bi is True, moments=[],
              loaded=lambda m: m.spec.bi_interaction is True and m.bi is True),
    # NFM: the exported deep_0 has the E more rows, the AUC is the restatement's in eval mode
    local=NS(args=["bi_interaction=1", "batch_norm=1"], line=None, exported=_bi_exported, value=True,
             ref=dict(bn=True, train=False)),
    off={"bi_interaction": False}, absent=["dl_bi_"], probe=_bi_probe, added=_bi_added)

# ---- bn: one model of each family
BN_KW = {"deepfm_pipeline": dict(C=13, V=3, S=8, E=8, cate_index_size=1000, hidden=[32, 16]),
         "dnn_pipeline": dict(C=13, V=3, S=8, E=8, cate_index_size=1000, hidden=[32, 16]),
         "dnn_multi_cate": dict(V=0, S=4, E=8, cate_index_size=1000, hidden=[32, 16],
                                multi_ranges=[[0, 5, "a"], [5, 6, "b"]]),
         "wdl": dict(C=13, S=8, E=8, cate_index_size=1000, hidden=[32, 16], Fw=4)}


def _bn_moved(P0, P):
    """The layer does matter, and every piece of its state moved."""
    assert np.abs(P[Bn.KEY % (2, "running_mean")] - P0[Bn.KEY % (2, "running_mean")]).max() > 100 * TOL
    assert np.abs(P[Bn.KEY % (1, "weight")] - P0[Bn.KEY % (1, "weight")]).max() > 100 * TOL


def _bn_drawn(p0, eng):
    assert (p0[Bn.KEY % (1, "weight")] == 1).all() and (p0[Bn.KEY % (1, "bias")] == 0).all()
    assert (p0[Bn.KEY % (1, "running_mean")] == 0).all() and (p0[Bn.KEY % (1, "running_var")] == 1).all()


def _bn_probe(eng, on):
    assert on or (eng.bn_groups == [] and not any(hasattr(eng, a) for a in ("bn_run", "bn_stat", "hx", "bn_ws")))


def _bn_params(pa):
    assert np.abs(pa[Bn.KEY % (1, "running_mean")]).max() > 0


def _bn_exported(P):
    assert P[Bn.KEY % (1, "running_var")].shape == (32,) and P[Bn.KEY % (2, "weight")].shape == (16,)
    assert np.abs(P[Bn.KEY % (1, "running_mean")]).max() > 0


BN = Case(
    key="bn", value=True, spec=lambda v: {"batch_norm": v}, keys=lambda v: [], KW=BN_KW,
    make_batch=Bn.make_batch,
    # gamma, beta off their initial 1 and 0
    init_params=lambda cfg, rng, v, L=0, A=0: Bn.init_params(cfg, L, A, True, rng, jitter=0.2),
    train_step=lambda cfg, P, opt, b, v, L=0, A=0, **o: Bn.train_step(cfg, P, opt, b, L, A, **o),
    forward=lambda cfg, P, b, v: Bn.forward_backward(cfg, P, b, bn=True, train=False),
    check=_bn_check, moved=_bn_moved,
    moment_keys=[Bn.KEY % (1, "weight")], bitwise=lambda name: name in ("dnn_pipeline", "deepfm_pipeline"),
    bitwise_keys=lambda name: Bn.bn_keys(R.make_cfg(name, **BN_KW[name]), running=False),
    withs={"the_cross_network_and_the_attention": [Run("dnn_multi_cate", 43, 15, "cross + afm + bn", init=dict(L=2, A=4),
                                                       ref=dict(L=2, A=4), spec=dict(afm_attention=4, cross_layers=2))]},
    # the statistics stay unweighted (a zero-weight row counts in mu and var), the loss is the weighted one
    weighted=_weighted(6, "deepfm_pipeline"),
    same_seed=SameSeed(model="wdl", value=True, drawn=_bn_drawn, v_keys=[Bn.KEY % (2, "bias")]),
    # (no predict: tests/test_gpu_bn.py's test_predict_uses_the_running_statistics)
    ckpt=Ckpt(args=dict(batch_norm=True, bn_momentum=0.2), built=lambda e: e.bn and e.spec.bn_momentum == 0.2,
              nonzero=True, params=_bn_params, moments=[Bn.KEY % (1, "weight"), Bn.KEY % (2, "bias")],
              loaded=lambda m: m.spec.batch_norm is True and m.bn and m.spec.bn_momentum == 0.2),
    local=NS(args=["batch_norm=1", "bn_momentum=0.3"], line=None, exported=_bn_exported, value=True, ref={}),
    off={"batch_norm": False}, absent=["dl_bn"], probe=_bn_probe,
    defaults=(("dnn_pipeline", "dense"), ("dnn_pipeline", "lazy"), ("wdl", "lazy")),
    # per layer: the step's stats, finish, sums, apply, bias row and Adam, predict's finish
    added=_removed(2 * ["dl_bn_stats", "dl_bn_fwd", "dl_bn_bwd_sums", "dl_bn_bwd_apply", "dl_bn_zero_bias_grad",
                        "dl_adam_dense", "dl_bn_fwd"]))

CASES = [CROSS, AFM, CCPM, CIN, AUTOINT, PNN, BI, BN]
