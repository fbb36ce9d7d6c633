"""Case tables and helpers of the envelope tests (test_envelope_cpu.py, test_gpu_envelope.py): the
embedding sizes, slot counts, cont-field counts and batch sizes at which the lookup, record and
pooling kernels take another instantiation or another route than the E = 8 / 16 shapes every other
test runs.

The dispatch arithmetic of csrc/embed.hip is restated here (fwd_arm, cont_arm, fused_gather_ok) so
the CPU file can assert that the tables reach every arm; the fixtures (parameters, batches, the
oracle's float32 trajectory and its float64 first-step gradient) are built once per case and
shared."""
import numpy as np

from deep_learning_amd.synthetic import make_batch
from oracle import ctr_ref as R

TOL = 1e-5           # logits, loss, parameters against the oracle (tests/test_gpu_parity.py)
REL = 1e-5           # a recovered gradient against float64, relative to that array's largest |G64|
# every first-step pre-activation (float64) is at least this far from 0, relative to the sum of its terms'
# magnitudes |x| |W| + |b|: 8 float32 roundings, past what a float32-accurate product of these widths loses,
# so the GPU's ReLU decides every unit as float64 does
RELU_MARGIN = 8 * 2.0 ** -24
HIDDEN = [32, 16]
N_IDS = 3000
B0 = 300
MULTI = [[0, 30, "a"], [30, 50, "b"]]
MAX_SLOTS, MAX_FM_CONT, TILE, FWD_GRID, BWD_WAVES = 128, 32, 16, 8192, 4096   # csrc/embed.hip

MODELS = {
    "deepfm_pipeline": dict(C=13, V=0, S=26),
    "wdl": dict(C=13, S=26, Fw=26),
    "deepfm_multi_cate": dict(V=4, S=8, multi_ranges=MULTI),
    "dnn_pipeline": dict(C=13, V=3, S=26),
    "dnn_multi": dict(C=13, V=2, S=12, multi_ranges=MULTI),
}
FM = ("deepfm_pipeline", "deepfm_multi_cate")
FM_CONT = ("deepfm_pipeline",)
SINGLE_VALUED = ("deepfm_pipeline", "wdl", "dnn_pipeline")


def kwargs(model, E, **over):
    kw = dict(MODELS[model], E=E, cate_index_size=N_IDS, hidden=list(HIDDEN))
    kw.update(over)
    return kw


def case_id(c):
    model, kw, B, mode = c
    return "%s-E%d-C%d-V%d-S%d-B%d-%s" % (model, kw["E"], kw.get("C", 0), kw.get("V", 0), kw["S"], B, mode)


# ---------------------------------------------------------------- the dispatch, restated
def slots(model, kw, deep=True):
    """Rows a sample looks up in the forward: FM cont + FM cate + (deep) cate."""
    S = kw["S"]
    fs = (kw.get("C", 0) if model in FM_CONT else 0) + S if model in FM else 0
    return fs + (S if deep else 0)


def limit_slots(model, kw):
    """What launch_embed_fwd holds against kMaxSlots (the deep slots counted whether looked up or not)."""
    S = kw["S"]
    return (kw.get("C", 0) if model in FM_CONT else 0) + 2 * S if model in FM else S


def fwd_arm(model, kw, deep=True):
    """(E, NPS) of the embed_fwd_kernel instantiation launch_embed_fwd picks."""
    E = kw["E"]
    rpi = 64 // (E // 4)
    n = slots(model, kw, deep)
    nps = -(-n // rpi) if n > 0 else 1
    if E == 16:
        return 16, min(max(nps, 1), 8)
    if E == 8:
        return 8, min(max(nps, 1), 4)
    return {4: (4, 2), 32: (32, 16), 64: (64, 32)}[E]


def cont_arm(model, kw):
    """(NC, kIt) of cont_bwd_kernel (the sorted and lazy backward of the FM cont rows), or None."""
    C = kw.get("C", 0)
    if model not in FM_CONT or C == 0:
        return None
    return (16, 4) if C <= 16 else (32, 1)


def bwd_passes(kw):
    """embed_bwd_kernel (atomic): rows a wave instruction adds, passes over the 32 register cont rows."""
    rpi = 64 // kw["E"]
    return rpi, -(-MAX_FM_CONT // rpi)


def fused_gather_ok(kw):
    """The shape part of CTREngine.fused_gather_rows / fused_gather_l0."""
    S, E = kw["S"], kw["E"]
    return E in (8, 16, 32, 64) and 0 < S <= 40 and (S * E) % 32 == 0


def gtab_ok(model, kw):
    """dl_embed_fwd_gtab_ok."""
    E = kw["E"]
    if E not in (8, 16):
        return False
    return -(-slots(model, kw, deep=False) // (64 // (E // 4))) <= 4


def fwd_tile_wraps(B):
    return -(-B // TILE) > FWD_GRID


def bwd_wave_wraps(B):
    return B > BWD_WAVES


# ---------------------------------------------------------------- case tables: (model, kw, B, mode)
def _cases(models_modes, Es, B=B0, **over):
    return [(m, kwargs(m, E, **over), B, mode) for m, modes in models_modes for E in Es for mode in modes]


ALL_MODES = ("atomic", "sorted", "lazy")
# 1. every embedding size, every table mode
SIZES = _cases([("deepfm_pipeline", ALL_MODES), ("wdl", ALL_MODES), ("deepfm_multi_cate", ALL_MODES),
                ("dnn_pipeline", ("lazy",)), ("dnn_multi", ("lazy",))], (4, 32, 64))
# 3. slot-count arms of the forward lookup: (E, C, S)
# (E = 64 at the 128-slot limit, C = 14 and S = 57, has 71 + 64 = 135 FM columns, past the 128 the output
# layer's kernel takes: refused at construction, HEAD_REFUSED; its all-slots form runs at the widest shape
# the head allows, C = 14 and S = 50: 114 slots, 128 FM columns)
SLOT_SHAPES = [(16, 13, 40), (16, 13, 48), (16, 13, 57), (16, 14, 57), (8, 13, 48), (4, 14, 57), (32, 14, 57),
               (64, 14, 50)]
SLOTS = [("deepfm_pipeline", kwargs("deepfm_pipeline", E, C=C, S=S), B0, mode)
         for E, C, S in SLOT_SHAPES for mode in ("atomic", "lazy")]
# E = 64 at the limit itself: without an FM part the 128 slots are the deep fields alone, every pass of the
# <64, 32> form holds a row and the block's whole slot table is filled
SLOTS += [("dnn_pipeline", kwargs("dnn_pipeline", 64, S=128), B0, mode) for mode in ("atomic", "lazy")]
ONE_SLOT_MORE = [("deepfm_pipeline", kwargs("deepfm_pipeline", E, C=13, S=58)) for E in (4, 8, 16, 32)]
MAX_FM_COLS = 128   # csrc/head.hip kHeadMaxFm
HEAD_REFUSED = [("deepfm_pipeline", kwargs("deepfm_pipeline", 64, C=14, S=57)),
                ("deepfm_pipeline", kwargs("deepfm_pipeline", 64, C=14, S=51)),
                ("deepfm_multi_cate", kwargs("deepfm_multi_cate", 64, S=63))]
# 4. cont-field arms
CONT = ([("deepfm_pipeline", kwargs("deepfm_pipeline", E, C=C, S=10), B0, mode)
         for C in (16, 17, 32) for E in (4, 16, 64) for mode in ("sorted", "lazy", "atomic")]
        + [("dnn_pipeline", kwargs("dnn_pipeline", 32, C=70, V=70, S=10), B0, mode) for mode in ("lazy", "atomic")])
ONE_CONT_MORE = [("deepfm_pipeline", kwargs("deepfm_pipeline", E, C=33, S=10)) for E in (4, 16, 64)]
# 5. batch edges (one step)
EDGE = ([(m, kwargs(m, E), B, "lazy") for m in ("deepfm_pipeline", "dnn_pipeline") for E in (4, 64)
         for B in (1, 15, 16, 17)]
        + [("deepfm_pipeline", kwargs("deepfm_pipeline", E), 4133, "atomic") for E in (4, 64)])
TINY = ("deepfm_pipeline", dict(C=2, V=0, S=2, E=4, cate_index_size=N_IDS, hidden=[8]), 131089, "atomic")
# 2. predict paths: (model, kw)
PREDICT = ([(m, kwargs(m, E)) for m in ("deepfm_pipeline", "dnn_pipeline") for E in (4, 32, 64)]
           + [(m, kwargs(m, 16, S=S)) for m in ("deepfm_pipeline", "dnn_pipeline") for S in (40, 42)])

# every case but TINY gets the gradient check: at 131,089 samples the float32 oracle's own sums are 2e-6 to
# 3e-5 of the largest gradient from float64 (40 seeds), so no fixture leaves the kernels room inside REL;
# TINY runs its forward and one step against the oracle at TOL
GRADIENT_CASES = SIZES + SLOTS + CONT + EDGE


def n_steps(c):
    return 1 if (c in EDGE or c is TINY) else 4


# ---------------------------------------------------------------- fixtures
def batches(model, kw, B, n, seed=11):
    """As test_gpu_parity._batches: the padding id and ids that alias the cont rows among the single-valued
    ids (as many as the shape has room for), multi-hot positions half padding."""
    out = []
    S, C = kw["S"], kw.get("C", 0)
    for i in range(n):
        b = make_batch(B, cont=C, vector=kw.get("V", 0), cate_fields=S, cate_index_size=kw["cate_index_size"],
                       seed=seed + i, wide_fields=kw.get("Fw", 0), cate_only=C == 0)
        k = min(4, S)
        b["cate_feats"][0, :k] = [0, 1, 5, 12][:k]       # padding id + ids that alias cont rows
        if B > 1:
            b["cate_feats"][1, :min(2, S)] = [27, 30][:min(2, S)]
        if "multi_ranges" in kw:
            rng = np.random.default_rng(seed + 100 + i)
            W = sum(e - s for s, e, _ in kw["multi_ranges"])
            multi = rng.integers(1, kw["cate_index_size"], size=(B, W))
            multi[rng.random((B, W)) < 0.5] = 0
            b["cate_feats"] = np.concatenate([b["cate_feats"], multi], 1)
        out.append(b)
    return out


def _key(model, kw, B, steps, seed):
    return (model, tuple(sorted((k, repr(v)) for k, v in kw.items())), B, steps, seed)


_REF = {}


def _seed(model, kw, B, steps):
    """The parameter seed: 42, or another for the shapes whose seed-42 fixture missed the CPU file's margins
    (test_envelope_cpu.py: the float32 oracle's gradient past REL / 4 of float64, or a pre-activation
    inside RELU_MARGIN)."""
    shape = (kw["E"], kw.get("C", 0), kw["S"], B)
    other = {"deepfm_pipeline": ((16, 14, 57, 300), (64, 13, 26, 15), (64, 13, 26, 4133)),
             "dnn_pipeline": ((64, 13, 128, 300),)}
    return 1 if shape in other.get(model, ()) else 42


def reference(model, kw, B, steps, seed=None):
    """The case's fixture, built once: initial parameters P0, the batches, the float32 oracle's
    trajectory (every step's logits and loss, step 0's forward, the final parameters), the float64
    gradient G64 of step 0 and the float32 one G32, and the smallest |pre-activation| of step 0 in float64."""
    if seed is None:
        seed = _seed(model, kw, B, steps)
    k = _key(model, kw, B, steps, seed)
    if k in _REF:
        return _REF[k]
    cfg = R.make_cfg(model, **kw)
    P0 = R.init_params(cfg, np.random.default_rng(seed))
    bs = batches(model, kw, B, steps)
    fw64 = R.forward(cfg, P0, bs[0], dtype=np.float64)
    G64, _ = R.backward(cfg, P0, bs[0], fw64, dtype=np.float64)
    h, margin = fw64["x0"], np.inf
    for i in range(len(cfg.hidden)):
        W, b = P0["deep_%d" % i].astype(np.float64), P0["deep_bias_%d" % i].astype(np.float64)
        pre = h @ W + b
        margin = min(margin, float((np.abs(pre) / (np.abs(h) @ np.abs(W) + np.abs(b))).min()))
        h = np.maximum(pre, 0)
    P = {k_: v.copy() for k_, v in P0.items()}
    opt = R.AdamTF1(cfg, P)
    zs, losses, fw0, G32 = [], [], None, None
    for i, b in enumerate(bs):
        fw = R.forward(cfg, P, b)
        G, _ = R.backward(cfg, P, b, fw)
        if i == 0:
            fw0, G32 = fw, G
        opt.apply(P, G)
        zs.append(fw["z"])
        losses.append(fw["loss"])
    _REF[k] = dict(cfg=cfg, P0=P0, batches=bs, fw64=fw64, G64=G64, G32=G32, margin=margin, fw0=fw0, zs=zs,
                   losses=losses, P=P)
    return _REF[k]


def case_reference(c):
    model, kw, B, _ = c
    return reference(model, kw, B, n_steps(c))


def grad_errors(G, G64):
    """Per parameter: max |G - G64| / max |G64| (0 where G64 is all zero and G is too)."""
    out = {}
    for k, g64 in G64.items():
        top = float(np.abs(g64).max())
        d = float(np.abs(np.asarray(G[k], np.float64).reshape(g64.shape) - g64).max())
        out[k] = d / top if top > 0 else (0.0 if d == 0 else np.inf)
    return out


# the float32 factor TF1 Adam applies to g - m (training_ops.cc: T(1) - beta1): m after the first step
ONE_MINUS_BETA1 = float(np.float32(1) - np.float32(0.9))


# ---------------------------------------------------------------- the catch-up window
HIST_WIN = 256     # rec.h kHistWin: steps of the alpha ring a block keeps in LDS
LAG_STEPS = 300    # batch 0's rows return at step 299
# (model, E, hist_len)
CATCH_UP = [("deepfm_pipeline", 16, 4096), ("deepfm_pipeline", 4, 4096), ("wdl", 16, 4096),
            ("deepfm_pipeline", 16, 512)]


def lag_batches(model, kw, B, n=LAG_STEPS, seed=7):
    """Batch 0 and batch n - 1 draw their ids from the lower half of the id range (their FM rows, the id
    plus C, included), the batches between from the upper half: the first batch's rows (and wide rows)
    lag n - 1 steps when they return."""
    half = kw["cate_index_size"] // 2
    out = []
    for i in range(n):
        b = make_batch(B, cont=kw.get("C", 0), cate_fields=kw["S"], cate_index_size=half - 32, seed=seed + i,
                       wide_fields=kw.get("Fw", 0))
        if 0 < i < n - 1:
            b["cate_feats"] = b["cate_feats"] + half
            if "wide_feats" in b:
                b["wide_feats"] = b["wide_feats"] + half
        out.append(b)
    return out
