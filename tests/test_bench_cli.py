"""bench.py's command line: a plain run is lean (timed steps and the result line only), --full adds the CPU
baselines and the parity check, --dump-outputs writes the last timed step's results, the same from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["status", "node_index", "evaluated_nodes", "feasible_nodes", "total_score"]
# SchedulingBasic on a small cluster: 2 timed steps of 40 pods after 1 warm-up step
SMALL = ["--gpus", "1", "--workload", "c1", "--nodes", "300", "--init-pods", "60", "--batch", "40",
         "--steps", "2", "--warmup", "1"]


def _import_bench():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import bench
    return bench


def test_dump_outputs_writes_every_result_field_as_float64(tmp_path):
    from ksg.abi import Result
    bench = _import_bench()
    rs = (Result * 3)()
    rs[0].status, rs[0].node_index, rs[0].evaluated_nodes, rs[0].feasible_nodes, rs[0].total_score = 0, 5, 9, 7, 463
    rs[1].status, rs[1].node_index = 1, -1
    rs[2].total_score = (1 << 40) + 1
    out = tmp_path / "nested" / "dump"
    bench.dump_outputs(str(out), rs)
    assert sorted(os.listdir(out)) == sorted(f + ".npy" for f in FIELDS)
    got = {f: np.load(out / (f + ".npy")) for f in FIELDS}
    for f in FIELDS:
        assert got[f].dtype == np.float64 and got[f].shape == (3,)
    assert [tuple(int(got[f][k]) for f in FIELDS) for k in range(3)] == [r.as_tuple() for r in rs]


def test_full_and_dump_outputs_are_options(monkeypatch):
    bench = _import_bench()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"])
    a = bench.parse()
    assert a.full is False and a.dump_outputs is None and a.steps == 3
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == "d"


def _run(args, dump):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + SMALL + args + ["--dump-outputs", str(dump)],
                       stdout=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0]), {f: np.load(os.path.join(dump, f + ".npy")) for f in FIELDS}


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    return _run([], tmp_path_factory.mktemp("plain"))


@pytest.mark.gpu
def test_plain_run_prints_the_headline_only(plain):
    line, dump = plain
    assert line["unit"] == "pods/s" and line["higher_is_better"] is True and line["dtype"] == "int64"
    assert line["steps"] == 2 and line["warmup"] == 1 and line["config"]["pods_per_step"] == 40
    assert line["value"] > 0 and line["ms_per_step"] > 0
    # value is the timed pods over the timed seconds, ms_per_step the same seconds over the steps (printed to
    # 1 us: up to 0.5 us off a step of well over 50 us)
    assert line["value"] == pytest.approx(40 / (line["ms_per_step"] * 1e-3), rel=1e-2)
    assert line["cpu_baseline"] is None and line["parity"] is None and "c5_100k" not in line
    for f in FIELDS:
        assert dump[f].dtype == np.float64 and dump[f].shape == (40,)
    assert int((dump["status"] == 0).sum()) == 40 and line["placed"] == 80
    assert ((dump["node_index"] >= 0) & (dump["node_index"] < 300)).all()


@pytest.mark.gpu
def test_full_run_adds_baseline_and_parity_and_computes_the_same(plain, tmp_path):
    line, dump = _run(["--full", "--cpu-seconds", "0.4"], tmp_path / "full")
    assert line["cpu_baseline"]["value"] > 0 and line["cpu_baseline"]["single_thread"]["value"] > 0
    # the baseline sample runs in chunks of 50 pods until its time budget: at least the first chunk is checked
    assert 50 <= line["parity"]["checked_pods"] <= 80 and line["parity"]["mismatches"] == 0
    assert "c5_100k" not in line  # the sub-record belongs to the default SchedulingBasic size only
    for f in FIELDS:
        assert np.array_equal(dump[f], plain[1][f]), f
