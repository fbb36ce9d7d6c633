"""bench.py as a program (GPU): a plain run prints the headline line alone and, with
--dump-outputs, writes the last timed step's arrays; --full adds the measurements beside it.
Small shapes (1,000-id fields, batch 512): the flow is under test, not the figures."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

pytestmark = pytest.mark.gpu

SMALL = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--vocab", "1000", "--batch", "512", "--age-steps", "2"]
FULL_ONLY = ("roofline", "cpu_baseline", "gather_north_star", "table_flush", "hbm_copy_measured", "kernels",
             "kernel_sum_us_per_step", "extra_workloads")


def _bench(*extra):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, os.path.abspath(bench.__file__)] + SMALL + list(extra), env=env,
                       capture_output=True, timeout=240)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    lines = p.stdout.decode().splitlines()
    assert len(lines) == 1, lines
    return json.loads(lines[0])


def test_plain_run_prints_the_headline_and_dumps_its_last_step(tmp_path):
    out = tmp_path / "dump"
    d = _bench("--dump-outputs", str(out))
    assert d["steps"] == 3 and d["warmup"] == 1 and d["n_gpus"] == 1 and d["full"] is False
    assert d["unit"] == "samples/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["ms_per_step"] > 0
    assert abs(d["value"] - 512 / (d["ms_per_step"] * 1e-3)) <= 1e-3 * d["value"]
    assert not [k for k in FULL_ONLY if k in d]
    got = {f[:-4]: np.load(out / f) for f in os.listdir(out)}
    assert {"logits", "scores", "loss", "table_rows", "first_order_rows", "deep_0", "deep_fm_weight"} <= set(got)
    assert all(a.dtype in (np.float32, np.float64) and np.isfinite(a).all() for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    assert got["logits"].shape == (512,) and got["table_rows"].shape == (26 * 1000 + 13, 16)
    assert np.allclose(got["scores"], 1.0 / (1.0 + np.exp(-got["logits"].astype(np.float64))), atol=1e-6)
    assert abs(float(got["loss"][0]) - d["loss"]) <= 1e-6
    assert got["table_rows"].any() and got["deep_0"].any()


def test_full_run_adds_the_other_measurements():
    d = _bench("--full", "--no-cpu-baseline", "--no-extra")
    assert d["full"] is True and d["steps"] == 3 and d["ms_per_step"] > 0
    assert d["roofline"]["kernel"] in d["kernels"] and d["kernel_sum_us_per_step"] > 0
    assert d["table_flush"]["us"] > 0 and d["hbm_copy_measured"]["GB/s"] > 0
    assert d["cpu_baseline"] is None and d["extra_workloads"] is None
