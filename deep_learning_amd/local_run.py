"""Drop-in for the reference CLI (local_run.py:12-91):

    python local_run.py ALG ACTION EPOCHS EMB_SIZE CATE_FEATS_SIZE PRINT_EVERY FEAT_CONF_DIR \
        TRAIN_PATH PREDICT_PATH MODEL_PB SAVE_CKPT MODEL_RESTORE RESTORE_CKPT [key=value ...]

The 13 positional arguments mean what they mean in the reference.  Optional
key=value overrides after them reach the hyper-parameters the reference
hard-codes (batch_size, hidden_units=400,400,400, learning_rate, l2_reg,
learning_rate_decay_steps/_rate, dropout_keep_deep=1,0.8,0.8,0.8, dropout_keep_fm=0.9,0.8, shuffle=0|1, shuffle_seed=N), so the
BASELINE configs (batch 65536, MLP [400]*3) are reachable from the same CLI.

pos_weight=2.5 weights the positives' loss terms and weight_key=NAME reads a per-sample loss weight
from the float [1] TFRecord feature NAME (tf.losses.log_loss's weights=, which the reference leaves
at 1); with weight_key, evaluation's logloss and calibration are weighted too.

cross_layers=N (dnn_pipeline, dnn_cate, dnn_multi, dnn_multi_cate) adds an N-layer Deep & Cross
network on the tower input, its output joining the tower's in the output layer.

afm_attention=A (the same four models) adds the attentional pairwise interactions of the reference's
test_model/AFM.py over the embedded fields, A attention units, its logit added to the tower's.

pnn=inner (the same four models) puts the inner-product layer of the reference's test_model/PNN.py in
front of the tower: the norm of a learned mix of the embedded fields, per unit of the first hidden layer.

batch_norm=1 bn_eps=1e-5 bn_momentum=0.1 (every model) normalises each hidden layer's pre-activation
over the batch before its ReLU (the reference's test_model/NFM.py); predict uses the running statistics.

bi_interaction=1 (dnn_pipeline, dnn_cate, dnn_multi, dnn_multi_cate) adds the Bi-Interaction pooling of the
reference's test_model/NFM.py, the sum of all pairwise products of the embedded fields, as E more columns
of the tower input; with batch_norm=1 the model is the reference's NFM.

ccpm_filters=C0,C1,.. (the same four models) adds the convolutional field interactions of the reference's
test_model/CCPM.py beside the tower: per value a 3x3 convolution of that many filters with ReLU and a 2x2
max-pool over the [embedding, field] map, then one more logit.

cin_layers=H1,H2,.. (the same four models) adds xDeepFM's Compressed Interaction Network beside the tower:
per value a layer of that many feature maps, each a learned sum of the element-wise products of the layer
below's maps with the embedded fields; every map is summed over the embedding into one more logit.

autoint_layers=L autoint_heads=Hn autoint_dim=D (the same four models; defaults 0, 2, 16; 0 layers: off) adds
AutoInt's interacting layers beside the tower: L stacked layers of multi-head self-attention over the
embedded fields (Hn heads on D columns) with a residual projection and a ReLU, then one more logit.

wide_optimizer=ftrl wide_lr=0.05 wide_l1=1e-3 wide_l2=0 (wdl: models/wdl.py reads them from its args)
train the wide weights with FTRL-proximal instead of Adam; L1 leaves most wide rows at exactly zero.

Two more overrides choose what evaluation reports (deep_learning_amd/metrics.py); without them
the output is the reference's: eval_metrics=auc,gauc,logloss,calibration (default auc) and
gauc_slot=K, the cate_feats column whose id groups the samples for GAUC (the user-id slot).
"""
import sys
import time

from .branches import BRANCHES, KEYWORDS, SIDE_MODELS
from .utils import data_loader as data_load
from .utils import my_utils

# local_run.py:47-68 dispatch (dnn_tensorboard is listed there but has no module in the reference)
ALGS = ("deepfm_pipeline", "deepfm_cate", "deepfm_multi_cate", "deepfm_multi", "dnn_cate", "dnn_pipeline",
        "dnn_multi_cate", "dnn_multi")


class ModelParams:
    def __init__(self, argv):
        self.alg_name = argv[1]
        self.action_type = argv[2]
        self.epochs = int(argv[3])
        self.embedding_size = int(argv[4])
        self.cate_feats_size = int(argv[5])
        self.num_batch_size = int(argv[6])
        self.feat_conf_path = argv[7]
        self.train_path = argv[8]
        self.predict_path = argv[9]
        self.model_pb = argv[10]
        self.save_model_checkpoint = argv[11]
        self.model_restore = int(argv[12])
        self.restore_model_checkpoint = argv[13]
        self.learning_rate = 0.001
        self.hidden_units = [512, 256, 128]
        self.dropout_keep_deep = [1, 1, 1, 1, 1]
        self.dropout_keep_fm = [1, 1]
        self.learning_rate_decay_steps = 10000000
        self.learning_rate_decay_rate = 0.9
        self.l2_reg = 0.00001
        self.batch_size = 1024
        self.shuffle = 1
        self.shuffle_seed = None
        spelt = {}      # the side options as given, for their refusals
        for kv in argv[14:]:
            k, v = kv.split("=", 1)
            if k == "hidden_units":
                self.hidden_units = [int(x) for x in v.split(",")]
            elif k in ("dropout_keep_deep", "dropout_keep_fm"):
                setattr(self, k, [float(x) for x in v.split(",")])
            elif k in ("batch_size", "learning_rate_decay_steps", "shuffle", "shuffle_seed"):
                setattr(self, k, int(v))
            elif k in ("learning_rate", "l2_reg", "learning_rate_decay_rate"):
                setattr(self, k, float(v))
            elif k == "gauc_slot":      # these two are stored only when given: the start-up dump stays as it is
                self.gauc_slot = int(v)
            elif k == "eval_metrics":
                self.eval_metrics = [m for m in v.split(",") if m]
            elif k == "pos_weight":     # sample weighting, stored only when given as well
                self.pos_weight = check_pos_weight(v)
            elif k == "weight_key":
                if not v:
                    raise SystemExit("weight_key= needs the name of a float [1] TFRecord feature")
                self.weight_key = v
            elif k in KEYWORDS:   # a side option of the tower (branches.py), stored only when given as well
                setattr(self, k, parse_side_option(KEYWORDS[k], k, v, self.alg_name))
                spelt[k] = kv
            elif k in ("wide_optimizer", "wide_lr", "wide_l1", "wide_l2"):   # stored only when given, too
                setattr(self, k, check_wide_option(k, v, self.alg_name))
            else:
                raise SystemExit("unknown override %s" % k)
        (self.cont_field_size, self.vector_feats_size, self.cate_field_size, self.multi_feats_size,
         self.multi_field_size, self.multi_feats_range) = my_utils.feat_size(self.feat_conf_path, self.alg_name)
        check_eval_options(getattr(self, "eval_metrics", None), getattr(self, "gauc_slot", None), self.cate_field_size)
        check_side_options(self, spelt)      # the fields' limits, known now that they are counted


EVAL_METRICS = ("auc", "gauc", "logloss", "calibration")


def check_pos_weight(v):
    """pos_weight=V as a float; refuses (SystemExit) anything not finite and > 0."""
    try:
        w = float(v)
    except ValueError:
        raise SystemExit("pos_weight=%s is not a number" % v)
    if not (w > 0.0 and w != float("inf")):
        raise SystemExit("pos_weight=%s must be finite and > 0" % v)
    return w


def parse_side_option(b, k, v, alg_name):
    """Keyword k=v of the side option b (a branches.py descriptor) as its value; refuses (SystemExit) what the
    text alone shows: a value its parser does not take, and switching the option on for a model other than
    the dnn_* ones.  (What depends on the fields is refused once they are counted: check_side_options.)"""
    value = b.parse(k, v)
    if k == b.name and value and b.phrases and alg_name not in SIDE_MODELS:
        raise SystemExit("%s=%s: %s the tower of %s only, not %s"
                         % (k, v, b.phrases[0], ", ".join(SIDE_MODELS), alg_name))
    return value


def check_side_options(mp, spelt):
    """Refuses (SystemExit) every side option that is on in the ModelParams mp and whose kernels do not take its
    fields, counted by now: the descriptor's refusal, which ModelSpec raises as a ValueError.  An option of one
    keyword is named as it was spelt (spelt: {keyword: "keyword=text"}), one of several by its name."""
    from .engine import FAMILIES
    E, F = mp.embedding_size, mp.cate_field_size + mp.multi_field_size
    for b in BRANCHES:
        values = b.values(mp)
        if not (values[0] and b.refusal):
            continue
        deep_in = (F * E + (mp.cont_field_size if FAMILIES[mp.alg_name]["cont"] else 0) + mp.vector_feats_size
                   + (E if getattr(mp, "bi_interaction", False) else 0))      # ModelSpec.deep_in
        why = b.refusal(F, E, deep_in, *values)
        if why:
            raise SystemExit("%s: %s" % (spelt[b.name] if len(b.keywords) == 1 else b.name, why))


def check_wide_option(k, v, alg_name):
    """wide_optimizer=adam|ftrl as a string, wide_lr / wide_l1 / wide_l2 as floats; refuses
    (SystemExit) what ModelSpec would: another optimizer name, ftrl for a model other than wdl,
    wide_lr <= 0, a negative wide_l1 / wide_l2, anything not finite."""
    if k == "wide_optimizer":
        if v not in ("adam", "ftrl"):
            raise SystemExit("wide_optimizer=%s must be adam or ftrl" % v)
        if v == "ftrl" and alg_name != "wdl":
            raise SystemExit("wide_optimizer=ftrl: only wdl has wide weights, not %s" % alg_name)
        return v
    try:
        x = float(v)
    except ValueError:
        raise SystemExit("%s=%s is not a number (wide_optimizer)" % (k, v))
    if not (x == x and abs(x) != float("inf") and (x > 0.0 if k == "wide_lr" else x >= 0.0)):
        raise SystemExit("%s=%s must be finite and %s 0 (wide_optimizer)" % (k, v, ">" if k == "wide_lr" else ">="))
    return x


def check_eval_options(eval_metrics, gauc_slot, cate_field_size):
    """Refuses (SystemExit, the CLI's way) an unknown metric, gauc without gauc_slot and a slot
    outside [0, cate_field_size)."""
    for m in eval_metrics or ():
        if m not in EVAL_METRICS:
            raise SystemExit("eval_metrics: unknown metric %s (known: %s)" % (m, ",".join(EVAL_METRICS)))
    if "gauc" in (eval_metrics or ()) and gauc_slot is None:
        raise SystemExit("eval_metrics: gauc needs gauc_slot=K (the cate_feats column that holds the group id)")
    if gauc_slot is not None and not 0 <= gauc_slot < int(cate_field_size):
        raise SystemExit("gauc_slot=%d outside [0, cate_field_size=%d)" % (gauc_slot, int(cate_field_size)))


def main(argv=None):
    argv = list(sys.argv if argv is None else argv)
    mp = ModelParams(argv)
    for key, value in mp.__dict__.items():
        print(key, "=", value)
    if mp.alg_name not in ALGS:
        print("alg_name = %s is error" % mp.alg_name)
        sys.exit(-1)
    alg_model = __import__("deep_learning_amd.models." + mp.alg_name, fromlist=["DeepModel"])
    eval_kw = {k: getattr(mp, k) for k in ("eval_metrics", "gauc_slot") if hasattr(mp, k)}
    if mp.action_type == "train":
        start_time = time.time()
        train_data = data_load.load_input_file(mp, mp.train_path, "train")
        predict_data = data_load.load_input_file(mp, mp.predict_path, "pred")
        m = alg_model.DeepModel(mp, train_data, predict_data)
        print("--------------train------------")
        m.fit(mp.num_batch_size)
        end_time = time.time()
        print("model training time: %.2f s" % (end_time - start_time))
        alg_model.predict(predict_data, mp.model_pb, **eval_kw)
    elif mp.action_type == "pred":
        print("--------------predict------------")
        predict_data = data_load.load_input_file(mp, mp.predict_path, "pred")
        alg_model.predict(predict_data, mp.model_pb, **eval_kw)
    else:
        print("action_type = %s is error !!!" % mp.action_type)


if __name__ == "__main__":
    main()
