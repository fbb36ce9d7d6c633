"""bench.py's bookkeeping (CPU): the PMC traffic it quotes comes only from a summary of the
same workload and id distribution, the calibrated backward bytes only for the case they were
measured on, and the vocab per workload follows BASELINE's configs (C4 = 100 M rows sharded)."""
import argparse
import json
import os

import numpy as np

import bench


def test_pmc_traffic_matches_workload_and_id_dist():
    got = bench.pmc_traffic("embed_bwd", 1, lazy=True, workload="c2", id_dist="uniform")
    assert got is not None
    d = json.load(open(os.path.join(bench.ROOT, got["source"])))
    assert d.get("workload", "c2") == "c2" and d.get("id_dist", "uniform") == "uniform"
    # no committed Zipf summary of C2's backward: nothing is quoted rather than uniform bytes
    z = bench.pmc_traffic("embed_bwd", 1, lazy=True, workload="c2", id_dist="zipf")
    if z is not None:
        assert json.load(open(os.path.join(bench.ROOT, z["source"]))).get("id_dist") == "zipf"
    assert bench.pmc_traffic("embed_bwd", 2, lazy=True) is None        # per-rank figures only at N = 1


def test_calibrated_backward_bytes_only_where_measured():
    cal = bench.bwd_calibrated("embed_bwd", 1, lazy=True, workload="c2", id_dist="uniform")
    assert cal is not None and cal["traffic_calibrated"] > 0
    d = json.load(open(os.path.join(bench.ROOT, cal["traffic_calibrated_source"])))
    # the calibration never exceeds the x2-everywhere figure and keeps every write
    assert d["write_bytes"] <= d["hbm_bytes_calibrated"] <= d["hbm_bytes_x2_everywhere"]
    for other in (dict(workload="c3"), dict(id_dist="zipf"), dict(lazy=False)):
        kw = dict(lazy=True, workload="c2", id_dist="uniform")
        kw.update(other)
        assert bench.bwd_calibrated("embed_bwd", 1, **kw) is None
    assert bench.bwd_calibrated("rec_gather", 1, lazy=True) is None


class _FakeEngine:
    """What dump_outputs reads of an engine, on the CPU: a lazy record table whose rows hold
    their own row number, logits / scores, two dense parameters (one above the per-array cap)."""
    lazy = True

    def __init__(self, n, E, B):
        import torch
        self.spec = argparse.Namespace(E=E, fm=True)
        self.N = n
        self.rec = torch.arange(n, dtype=torch.float32)[:, None].repeat(1, 3 * E + 4)
        self.z = torch.linspace(-1, 1, B + 8)
        self.score = torch.sigmoid(self.z)
        self.flushed = 0

    def dense_params(self):
        return {"deep_0": np.ones((3, 5), np.float32),
                "big": np.arange(bench.DUMP_MAX_ELEMS + 10, dtype=np.float32)}

    def flush(self):
        self.flushed += 1


def test_dump_outputs_files_are_float_bounded_and_repeatable(tmp_path):
    n, E, B = bench.DUMP_TABLE_ROWS * 2, 4, 64
    dirs = [str(tmp_path / "a"), str(tmp_path / "b")]
    for d in dirs:
        eng = _FakeEngine(n, E, B)
        bench.dump_outputs(eng, B, 0.625, d, sharded=False)
        assert eng.flushed == 1                       # rows are read caught up
    got = {f[:-4]: np.load(os.path.join(dirs[0], f)) for f in sorted(os.listdir(dirs[0]))}
    assert set(got) == {"logits", "scores", "loss", "deep_0", "big", "table_rows", "first_order_rows"}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    assert got["logits"].shape == (B,) and got["loss"].tolist() == [0.625]
    assert got["big"].shape == (bench.DUMP_MAX_ELEMS,)                  # a seeded sample of the elements
    rows = got["table_rows"]
    assert rows.shape == (bench.DUMP_TABLE_ROWS, E) and (np.diff(rows[:, 0]) > 0).all()
    assert (got["first_order_rows"] == rows[:, 0]).all()                # the same rows' first-order weights
    for name, a in got.items():                                         # the same sample every run
        assert np.array_equal(a, np.load(os.path.join(dirs[1], name + ".npy"))), name
    # the sharded engine: this rank's step outputs only
    bench.dump_outputs(_FakeEngine(n, E, B), B, 0.5, str(tmp_path / "s"), sharded=True)
    assert sorted(os.listdir(tmp_path / "s")) == ["logits.npy", "loss.npy", "scores.npy"]


def test_vocab_per_workload():
    a = argparse.Namespace(vocab=None)
    assert bench.vocab_for("c2", a, sharded=False) == 1_000_000
    assert bench.vocab_for("c5", a, sharded=True) == 1_000_000
    v = bench.vocab_for("c2", a, sharded=True)          # C4: 100 M rows over the 26 fields
    assert v * 26 >= 100_000_000 > (v - 1) * 26
    assert bench.vocab_for("c2", argparse.Namespace(vocab=7), sharded=True) == 7
