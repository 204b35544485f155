"""bench.py's contract with the driver: one JSON line on stdout with the required keys; a plain run times exactly --steps
steps and its --dump-outputs arrays are the last step's results; with --full, `roofline` and (unless switched off)
`cpu_baseline`, and the N > 1 code path (sc_allgather_paths + its consistency checks) driven at world size 1."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "dtype", "config")
REQUIRED = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
            "dtype", "data", "config", "roofline")


def _bench(args, env=None):
    e = dict(os.environ)
    e.update(env or {})
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + args, cwd=ROOT, env=e, capture_output=True,
                       text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, lines            # exactly one line on stdout
    return json.loads(lines[0])


def _run(extra, env=None):
    return _bench(["--steps", "4", "--warmup", "2", "--only-main-map", "--replan-frames", "0", "--repeats", "3", "--full"] + extra, env)


def test_bench_plain_run_and_dump(tmp_path, oracle):
    """A plain run: the headline only, --steps timed steps, and the arrays of the last timed step (step 3 of one call of 4:
    grid SEED_GRID + 3, query block 3) written as float64 -- equal to the CPU oracle's EDT and A* on the same inputs."""
    import numpy as np
    from sea_current_amd import synth
    d = _bench(["--steps", "4", "--warmup", "2", "--dump-outputs", str(tmp_path)])
    for k in HEADLINE:
        assert k in d, k
    assert d["steps"] == 4 and d["repeats"] == 1 and d["config"]["steps_per_call"] == 4 and d["ms_per_step"] > 0
    assert abs(d["value"] - d["config"]["queries_total"] * 1e3 / d["ms_per_step"]) / d["value"] < 1e-6
    assert not {"roofline", "cpu_baseline", "value_depth1", "kernels", "other_maps", "configs2"} & set(d)
    files = sorted(os.listdir(tmp_path))
    assert files == ["cost.npy", "d2.npy", "len.npy", "path.npy", "status.npy"], files
    assert sum(os.path.getsize(tmp_path / f) for f in files) <= 64 << 20
    got = {f[:-4]: np.load(tmp_path / f) for f in files}
    assert all(a.dtype == np.float64 for a in got.values())
    occ = synth.salt_grid(1024, 1024, 0.20, seed=synth.SEED_GRID + 3)
    d2 = oracle.edt(occ)
    assert np.array_equal(got["d2"], d2)
    s, g = synth.queries(d2 >= 1, 1024, first=3 * 1024)
    ref = oracle.astar_batch(d2, s, g, Lmax=4096, nthreads=16)
    for k in ("status", "cost", "len"):
        assert np.array_equal(got[k], ref[k]), k
    for q in range(1024):
        n = int(ref["len"][q])
        assert np.array_equal(got["path"][q, :n], ref["path"][q, :n]) and (got["path"][q, n:] == -1).all(), q


def test_bench_line_contract():
    d = _run(["--cpu-seconds", "1"])
    for k in REQUIRED:
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 4 and d["warmup"] == 2 and d["higher_is_better"] is True and d["scaling"] == "weak"
    assert d["vs_baseline"] is None and d["unit"] == "plans/s" and d["value"] > 0
    assert abs(d["value"] - d["config"]["queries_total"] * 1e3 / d["ms_per_step"]) / d["value"] < 1e-6
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9 and r["frac"] > 0.3
    c = d["cpu_baseline"]
    assert c["kind"] == "port" and c["cores"] >= 1 and c["value"] > 0 and c["gpu_matches_cpu_on_sample"] is True
    # the steps of a call are distinct batches (own grid, own queries): a step other than step 0 is checked against the oracle too
    assert c["gpu_matches_cpu_on_step"]["step_of_the_call"] == 3 and c["gpu_matches_cpu_on_step"]["matches"] is True
    assert d["repeats"] >= 3 and d["value_min"] <= d["value"] <= d["value_max"] and len(d["ms_per_region"]) == d["repeats"]
    assert d["config"]["queries_per_launch"] == 4 * d["config"]["queries_per_gpu"] and d["value_depth1"] > 0
    assert d["per_query_depth1"]["kilocycles_max"] >= d["per_query_depth1"]["kilocycles_p99"] >= d["per_query_depth1"]["kilocycles_p50"] > 0


def test_bench_gather_path_world1():
    d = _run(["--no-cpu-baseline"], env={"SC_BENCH_FORCE_DIST": "1"})
    g = d["gather"]
    assert g["consistent_on_all_ranks"] is True and g["truncated"] == 0
    assert 0 < g["bytes_received_per_rank_per_step"] < g["fixed_stride_bytes_per_rank_per_step"]
