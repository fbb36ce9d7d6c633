"""CPU checks of the dense side-branch parameter groups (deep_learning_amd/param_groups.py): every
layout's pack / unpack both ways at tiny sizes, bit for bit and in the reference's shapes, its size refusal;
and the three refusals ModelSpec shares between cross_layers, afm_attention, pnn, bi_interaction and
ccpm_filters, in each option's own words."""
import re
from functools import partial

import numpy as np
import pytest

from deep_learning_amd import param_groups as G

E, F, A, FILTERS, L, D0, D1 = 8, 3, 4, (2,), 2, 20, 5
ROWS = np.random.default_rng(5).permutation(D0)
CCPM_SHAPES = G.ccpm_shapes([(E, F, 1), (E // 2, F // 2, FILTERS[0])])

# name -> (pack, unpack, {key: reference shape}, a wrong-sized entry, its refusal)
LAYOUTS = {
    "cross": (partial(G.cross_pack, L=L, D0=D0, rows=ROWS), partial(G.cross_unpack, L=L, D0=D0, rows=ROWS),
              {k: (D0, 1) for k in G.cross_keys(L)},
              ("cross_bias_1", (D0 - 1, 1)), "cross_bias_1 holds 19 values for 20 tower-input columns"),
    "afm": (partial(G.afm_pack, E=E, A=A), partial(G.afm_unpack, E=E, A=A),
            {"attention_p": (E, 1), "attention_h": (1, A), "attention_b": (1, A), "attention_w": (E, A)},
            ("attention_h", (1, A + 1)), "attention_h holds 5 values, not 1 x 4"),
    "ccpm": (partial(G.ccpm_pack, shapes=CCPM_SHAPES), partial(G.ccpm_unpack, shapes=CCPM_SHAPES),
             {"ccpm_out.kernel": (4 * 1 * 2, 1), "ccpm_conv_0.kernel": (3, 3, 1, 2), "ccpm_conv_0.bias": (2,)},
             ("ccpm_conv_0.bias", (3,)), "ccpm_filters: ccpm_conv_0.bias holds 3 values, not 2"),
    "pnn": (partial(G.pnn_pack, D1=D1, F=F), partial(G.pnn_unpack, D1=D1, F=F),
            {"product-quadratic-inner": (D1, F)},
            ("product-quadratic-inner", (F, D1)), "product-quadratic-inner has shape (3, 5), not (5, 3)"),
}


def _params(shapes, seed):
    rng = np.random.default_rng(seed)
    return {k: rng.standard_normal(shp).astype(np.float32) for k, shp in shapes.items()}


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_pack_unpack_round_trip(name):
    pack, unpack, shapes, (bad_key, bad_shape), message = LAYOUTS[name]
    n = sum(int(np.prod(shp)) for shp in shapes.values())
    assert (ROWS != np.arange(D0)).any()
    P = _params(shapes, 1)
    v = pack(P)
    assert v.dtype == np.float32 and v.shape == (n,)
    back = unpack(v)
    assert list(back) == list(shapes)
    for k, shp in shapes.items():
        assert back[k].dtype == np.float32 and back[k].shape == shp and np.array_equal(back[k], P[k]), k
        assert not np.shares_memory(back[k], v), k
    v = np.arange(n, dtype=np.float32)
    assert np.array_equal(pack(unpack(v)), v)
    bad = dict(P, **{bad_key: np.zeros(bad_shape, np.float32)})
    with pytest.raises(ValueError, match="^" + re.escape(message) + "$"):
        pack(bad)


def test_the_vectors_orders():
    """cross: [c | w_0 w_1 | b_0 b_1], every part in x0's column order (rows: the reference row of each
    column); afm: [p | h | b | W]; ccpm: [p | K_0 | b_0]; pnn: theta row-major."""
    P = _params(LAYOUTS["cross"][2], 2)
    v = LAYOUTS["cross"][0](P).reshape(2 * L + 1, D0)
    for i, k in enumerate(["cross_res", "cross_layer_0", "cross_layer_1", "cross_bias_0", "cross_bias_1"]):
        assert np.array_equal(v[i], P[k][ROWS, 0]), k
    for name in ("afm", "ccpm", "pnn"):
        P = _params(LAYOUTS[name][2], 3)
        assert np.array_equal(LAYOUTS[name][0](P), np.concatenate([P[k].reshape(-1) for k in LAYOUTS[name][2]]))


def test_batch_norm_vector():
    """[gamma | beta] of hidden layer l under batch_norm_{l+1}.weight / .bias; absent running statistics
    take their default, a vector of another size is refused."""
    P = {"batch_norm_2.weight": np.arange(3, dtype=np.float32), "batch_norm_2.bias": -np.arange(3, dtype=np.float32)}
    v = G.bn_pack(P, 1, 3)
    assert v.dtype == np.float32 and np.array_equal(v, [0, 1, 2, 0, -1, -2])
    back = G.bn_unpack(v, 1, 3)
    assert list(back) == list(P) and all(np.array_equal(back[k], P[k]) for k in P)
    assert np.array_equal(G.bn_vec(P, 1, "running_var", 3, 1.0), np.ones(3, np.float32))
    with pytest.raises(ValueError, match=r"^batch_norm_2\.weight holds 3 values for 4 units$"):
        G.bn_pack(P, 1, 4)
    with pytest.raises(KeyError):
        G.bn_pack(P, 0, 3)


# --------------------------------------------------------------------------- ModelSpec's shared refusals
KW = dict(C=5, V=3, S=6, E=8, cate_index_size=300, hidden=[16, 8])
MODELS = "dnn_pipeline, dnn_cate, dnn_multi, dnn_multi_cate"
# option -> (its argument, who joins the tower, why not bf16, why not tower-input dropout)
OPTIONS = {
    "cross_layers": (2, "the cross network joins", "the cross network reads the f32 tower input",
                     "the cross network reads the undropped input"),
    "afm_attention": (4, "the attentional interactions join", "the branch reads the f32 tower input",
                      "the branch reads the undropped fields"),
    "pnn": ("inner", "the product layer feeds",
            "the product layer reads the f32 tower input and finishes the f32 first layer",
            "the product layer reads the undropped fields"),
    "bi_interaction": (True, "the Bi-Interaction pooling feeds", "the pooling reads and extends the f32 tower input",
                       "the pooling's backward reads the undropped fields"),
    "ccpm_filters": ((2,), "the convolutional interactions join", "the branch reads the f32 tower input",
                     "the branch reads the undropped fields"),
}


@pytest.mark.parametrize("opt", list(OPTIONS))
def test_model_spec_shared_refusals(opt):
    from deep_learning_amd.engine import ModelSpec
    value, joins, bf16, drop = OPTIONS[opt]
    on = {opt: value}
    for model in ("deepfm_pipeline", "wdl", "dnn"):
        with pytest.raises(ValueError) as e:
            ModelSpec(model, **on, **dict(KW, Fw=4 if model == "wdl" else 0))
        assert str(e.value) == "%s: %s the tower of %s only, not %s" % (opt, joins, MODELS, model)
    with pytest.raises(ValueError) as e:
        ModelSpec("dnn_pipeline", tower="bf16", **on, **KW)
    assert str(e.value) == "%s: not supported with tower='bf16' (%s)" % (opt, bf16)
    with pytest.raises(ValueError) as e:
        ModelSpec("dnn_pipeline", dropout_keep_deep=[0.9, 1, 1], **on, **KW)
    assert str(e.value) == ("%s: not supported with tower-input dropout (dropout_keep_deep[0] < 1 rewrites x0 in "
                            "place; %s)" % (opt, drop))
    sp = ModelSpec("dnn_pipeline", dropout_keep_deep=[1, 1, 0.9], **on, **KW)     # dropout elsewhere is fine
    assert getattr(sp, opt) == value
