"""CPU checks of the side options' descriptor table (deep_learning_amd/branches.py): around every limit,
ModelSpec (ValueError) and local_run (SystemExit) refuse the same cells in the same words; both engines' "not
supported by" refusals name every option; _spec_from_args hands every option over and nothing else."""
import types

import pytest

from deep_learning_amd import branches as Br
from deep_learning_amd.engine import ModelSpec

FS, ES = (1, 2, 64, 65), (4, 8, 16, 32, 64)
# option -> its values around the limits: the limit itself, one past it, one below the minimum
VALUES = {
    "cross_layers": [dict(cross_layers=v) for v in (1, Br.CROSS_MAX_LAYERS, Br.CROSS_MAX_LAYERS + 1)],
    "afm_attention": [dict(afm_attention=v) for v in (1, Br.AFM_MAX_ATT, Br.AFM_MAX_ATT + 1)],
    "ccpm_filters": [dict(ccpm_filters=v) for v in ((Br.CCPM_MAX_FILTERS,), (2,) * Br.CCPM_MAX_LAYERS,
                                                    (Br.CCPM_MAX_FILTERS + 1,), (2,) * (Br.CCPM_MAX_LAYERS + 1), (0,))],
    # at 64 fields (64,) holds exactly CIN_MAX_WEIGHTS; (64, 1), 4096 more, is the next count the limits on the
    # maps leave reachable
    "cin_layers": [dict(cin_layers=v) for v in ((1,), (Br.CIN_MAX_MAPS,), (Br.CIN_MAX_MAPS, 1), (Br.CIN_MAX_MAPS + 1,),
                                                (2,) * (Br.CIN_MAX_LAYERS + 1), (0,))],
    "autoint_layers": [dict(autoint_layers=L, autoint_heads=Hn, autoint_dim=D)
                       for L, Hn, D in ((1, 1, 8), (Br.AUTOINT_MAX_LAYERS, 4, 32), (Br.AUTOINT_MAX_LAYERS + 1, 2, 16),
                                        (-1, 2, 16), (1, 3, 16), (1, 2, 64), (1, 4, 4))],
    "pnn": [dict(pnn="inner")],
    "bi_interaction": [dict(bi_interaction=True)],
}
ALONE = dict({k: v[0] for k, v in VALUES.items()}, batch_norm=dict(batch_norm=True))


def test_the_table():
    assert [b.name for b in Br.BRANCHES] == ["cross_layers", "afm_attention", "ccpm_filters", "cin_layers",
                                             "autoint_layers", "pnn", "bi_interaction", "batch_norm"]
    assert set(VALUES) == {b.name for b in Br.BRANCHES if b.refusal} and set(ALONE) == {b.name for b in Br.BRANCHES}
    assert Br.cin_weights(64, (Br.CIN_MAX_MAPS,)) == Br.CIN_MAX_WEIGHTS < Br.cin_weights(64, (Br.CIN_MAX_MAPS, 1))
    for b in Br.BRANCHES:
        assert list(b.keywords)[0] == b.name and not b.values(types.SimpleNamespace())[0]      # off by default


def _text(v):
    return ",".join(map(str, v)) if isinstance(v, tuple) else "1" if v is True else str(v)


def _argv(root, alg, F, E, opts, floats=0):
    conf = root / ("conf_%d_%d" % (floats, F))
    if not conf.exists():
        conf.mkdir()
        lines = ["f%d\tx\tfloat" % i for i in range(floats)] + ["c%d\tx\tstring" % i for i in range(F)]
        (conf / "dnn.conf").write_text("\n".join(lines) + "\n")
    return (["local_run.py", alg, "train", "1", str(E), "3000", "3", str(conf), "tr/", "pr/", "pb", "ck", "0", "ck"]
            + ["%s=%s" % (k, _text(v)) for k, v in opts.items()])


def _both(root, alg, F, E, opts, floats=0):
    """(ModelSpec's ValueError or None, local_run's SystemExit or None) for one cell."""
    from deep_learning_amd.local_run import ModelParams
    ve = se = None
    try:
        ModelSpec(alg, C=floats, S=F, E=E, hidden=[8], **opts)
    except ValueError as e:
        ve = str(e)
    try:
        ModelParams(_argv(root, alg, F, E, opts, floats))
    except SystemExit as e:
        se = str(e)
    return ve, se


def _limits(b):
    """The numbers of the option's limits (the module constants of its prefix), as its refusal prints them."""
    prefix = {"bi_interaction": "BI_", "pnn": "PNN_"}.get(b.name, b.key.upper() + "_")
    out = []
    for k, v in vars(Br).items():
        if k.startswith(prefix) and k.isupper() and not isinstance(v, str):
            out.append(Br._slashes(v) if isinstance(v, tuple) else str(v))
    assert out, b.name
    return out


@pytest.mark.parametrize("name", list(VALUES))
def test_model_spec_and_local_run_refuse_the_same_cells(tmp_path, capsys, name):
    b = Br.KEYWORDS[name]
    refused = accepted = 0
    for opts in VALUES[name]:
        for F in FS:
            for E in ES:
                ve, se = _both(tmp_path, "dnn_cate", F, E, opts)
                cell = "%r on %d fields of size %d: ModelSpec %r, local_run %r" % (opts, F, E, ve, se)
                assert (ve is None) == (se is None), cell
                if ve is None:
                    accepted += 1
                    continue
                refused += 1
                assert name in ve and name in se, cell
                if " got " in se:     # the fields' refusal: one function, one wording after the option's spelling
                    assert ve.split(": ", 1)[1] == se.split(": ", 1)[1], cell
                    assert all(n in ve for n in _limits(b)), cell
                else:                 # the text alone was enough for local_run: its limit is ModelSpec's
                    shown = [n for n in _limits(b) if n in se]
                    assert shown and all(n in ve for n in shown), cell
    assert refused and accepted, name
    capsys.readouterr()


def test_the_cont_columns_count_for_the_cross_network(tmp_path, capsys):
    """dnn_pipeline's 13 cont columns beside 64 fields of size 16: 1037 tower-input columns, 13 too many; dnn_cate
    reads no cont column and takes the same fields."""
    ve, se = _both(tmp_path, "dnn_pipeline", 64, 16, dict(cross_layers=1), floats=13)
    assert "got 1 on 1037" in ve and ve.split(": ", 1)[1] == se.split(": ", 1)[1]
    assert _both(tmp_path, "dnn_cate", 64, 16, dict(cross_layers=1), floats=13) == (None, None)
    ve, se = _both(tmp_path, "dnn_cate", 64, 16, dict(cross_layers=1, bi_interaction=True))
    assert "got 1 on 1040" in ve and ve.split(": ", 1)[1] == se.split(": ", 1)[1]
    capsys.readouterr()


@pytest.mark.parametrize("name", list(ALONE))
def test_both_engines_name_every_option(monkeypatch, name):
    """Before anything touches a device: ShardedCTREngine's own refusal, and CTREngine's for any other subclass."""
    import torch

    from deep_learning_amd import engine as eng_mod
    from deep_learning_amd.shard import ShardedCTREngine
    spec = ModelSpec("dnn_pipeline", C=13, V=3, S=8, E=8, hidden=[32, 16], **ALONE[name])
    with pytest.raises(ValueError, match="^%s: not supported by ShardedCTREngine \\(" % name):
        ShardedCTREngine(spec, 64, types.SimpleNamespace(world=1, rank=0))
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(eng_mod._lib, "lib", lambda: None)
    with pytest.raises(ValueError, match="^%s: not supported by Other \\(" % name):
        type("Other", (eng_mod.CTREngine,), {})(spec, 64)


def _args(**over):
    return types.SimpleNamespace(hidden_units=[32, 16], embedding_size=8, cate_feats_size=3000, learning_rate=0.001,
                                 l2_reg=1e-5, learning_rate_decay_steps=1000, learning_rate_decay_rate=0.9,
                                 vector_feats_size=3, cate_field_size=8, cont_field_size=13, **over)


def test_spec_from_args_round_trip():
    from deep_learning_amd.models._ctr_model import _spec_from_args
    direct = ModelSpec("dnn_pipeline", E=8, cate_index_size=3000, hidden=[32, 16], lr=0.001, l2=1e-5, decay_steps=1000.0,
                       decay_rate=0.9, V=3, S=8, C=13)
    plain = vars(_spec_from_args("dnn_pipeline", _args()))
    assert plain == vars(direct)
    assert {k: plain[k] for k in Br.KEYWORDS} == {k: d for b in Br.BRANCHES for k, d in b.keywords.items()}
    for name, opts in ALONE.items():
        got = vars(_spec_from_args("dnn_pipeline", _args(**{k: list(v) if isinstance(v, tuple) else v
                                                            for k, v in opts.items()})))
        assert {k: got[k] for k in opts} == opts, name
        assert {k: v for k, v in got.items() if k not in opts} == {k: v for k, v in plain.items() if k not in opts}, name
