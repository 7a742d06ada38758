"""The ONE stdout line of bench.py (the driver's record of a round) stays parsable.

Round 4's line carried every secondary leg and grew to ~30 KB: the driver's bounded tail cut
it and `BENCH_r04.parsed` was null.  The line is now compact (< 4 KB: headline, roofline,
cpu_baseline, one figure per secondary leg); the full record goes to a side file / stderr."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REQUIRED = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
            "scaling", "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline")


def check_line(line):
    assert len(line) < 4096, len(line)
    d = json.loads(line)
    for k in REQUIRED:
        assert k in d, k
    assert d["config"]["workload"].startswith("compressible sedov")
    rf = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic", "kernel", "kernel_avg_ms"):
        assert k in rf, k
    assert rf["frac"] > 0 and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-4 * rf["frac"] + 1e-12
    cb = d["cpu_baseline"]
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in cb, k
    return d


def test_bench_whole_script_on_the_emulator(tmp_path):
    """the driver's exact flags with --full (+ a tiny grid and every secondary leg scaled down)
    through bench.main() on the host emulator: ONE stdout line, < 4 KB, with roofline, cpu_baseline
    and targets; the full record lands in the side file"""
    env = dict(os.environ, PYRO_TEST_WORKERS="0")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "run_bench_emu.py"),
                        "--gpus", "1", "--steps", "20", "--warmup", "5", "--nx", "64", "--also-div", "64",
                        "--cpu-sample-nx", "32", "--cpu-seconds", "1", "--full"],
                       capture_output=True, text=True, timeout=900, env=env, cwd=str(tmp_path))
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    d = check_line(lines[0])
    assert d["steps"] == 20 and d["warmup"] == 5 and d["n_gpus"] == 1
    t = d["targets"]
    for k in ("sedov_exact", "sedov_developed", "sedov_4096", "sedov_8192", "advection_2048", "advection_8192",
              "mg_4096", "incompressible_2048", "pyro_driver"):
        assert k in t and "error" not in t[k], (k, t.get(k))
    for k, v in t["pyro_driver"].items():
        assert "error" not in v, (k, v)
    full = json.load(open(os.path.join(ROOT, d["full_record"])))
    assert "also" in full and abs(full["value"] - d["value"]) <= 1e-5 * d["value"]
    assert "[bench also] multigrid:" in p.stderr


@pytest.mark.parametrize("name", ["r04_bench_default.json"])
def test_compact_line_of_a_full_hardware_record(name):
    """a full record as a GPU box produced it (round 4's 30 KB line) through compact_line"""
    import bench
    full = json.load(open(os.path.join(ROOT, "profiles", name)))
    d = check_line(bench.compact_line(full, "gpurun_out/bench_full.json"))
    assert d["roofline"]["kernel"] == "k_ctu_wave" and d["roofline"]["traffic"] > 0
    assert d["targets"]["sedov_8192"]["frac"] > 0.1 and d["targets"]["advection_2048"]["step_frac"] > 0.3
    assert d["targets"]["mg_4096"]["value"] > 1000


def test_compact_line_with_eight_ranks():
    """the N = 8 line carries the per-rank table and still fits"""
    import bench
    full = json.load(open(os.path.join(ROOT, "profiles", "r04_bench_default.json")))
    full.pop("also")
    cols = ("kernel_ms", "halo_wait_ms", "halo_sync_ms", "allreduce_ms", "stream_ms_per_step", "rows",
            "col_strips", "rows_per_strip", "row_strips", "overlap", "wavefronts")
    table = {c: [1.2345678901 + i for i in range(8)] for c in cols}
    full["n_gpus"] = 8
    full["ranks"] = {"per_rank": table, "min": {c: 1.0 for c in cols}, "max": {c: 9.0 for c in cols},
                     "note": "x" * 600, "predicted_ms_per_step": 1.4, "predicted_source": "DESIGN"}
    full["config"]["scale_check"] = {"ok": True, "nx": 2048, "steps": 12, "note": "y" * 500}
    d = check_line(bench.compact_line(full, None))
    assert len(d["ranks"]["kernel_ms"]) == 8


PLAIN = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
         "dtype", "config")


def run_plain(cwd, *extra):
    env = dict(os.environ, PYRO_TEST_WORKERS="0")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "run_bench_emu.py"),
                        "--gpus", "1", "--steps", "7", "--warmup", "2", "--nx", "64"] + list(extra),
                       capture_output=True, text=True, timeout=600, env=env, cwd=str(cwd))
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


def test_bench_plain_run_and_dump_outputs(tmp_path):
    """without --full: the headline alone (no roofline, cpu_baseline or secondary legs, no side
    file); --dump-outputs writes the state after the last timed step and the dt of every timed
    step, the same from run to run"""
    import bench
    outs = []
    for k in range(2):
        d = run_plain(tmp_path, "--dump-outputs", str(tmp_path / f"out{k}"))
        for key in PLAIN:
            assert key in d, key
        assert d["steps"] == 7 and d["warmup"] == 2 and d["unit"] == "cell-updates/s"
        assert d["dtype"] == "f64" and d["higher_is_better"] is True
        assert abs(d["value"] - 64 * 64 / (d["ms_per_step"] * 1e-3)) <= 1e-4 * d["value"]
        for key in ("roofline", "roofline_fp64", "cpu_baseline", "targets", "full_record"):
            assert key not in d, key
        outs.append({n: np.load(str(tmp_path / f"out{k}" / (n + ".npy")))
                     for n in ("dt", "state_center", "state_sample")})
    a, b = outs
    assert a["dt"].shape == (7,) and a["dt"].dtype == np.float64 and (a["dt"] > 0).all()
    assert a["state_center"].shape == (64, 64, 4) and a["state_sample"].shape == (64, 64, 4)
    for n in a:
        assert np.array_equal(a[n], b[n]), n
    # the dumped cells are those of the state after warm-up + steps steps
    from pyro2_amd.compressible.problems.sedov import sedov_state
    ic = sedov_state(64, 64, 4, 0.0, 1.0, 0.0, 1.0, 1.4, 0.01, 4)[4:-4, 4:-4]
    assert np.abs(a["state_center"] - ic).max() > 0
    wr, wc, sr, sc = bench.dump_selection(64, 64)
    assert np.array_equal(a["state_center"], a["state_sample"][np.ix_(np.searchsorted(sr, wr),
                                                                      np.searchsorted(sc, wc))])


def test_dump_outputs_stay_small():
    """--dump-outputs at the headline size writes < 64 MB"""
    import bench
    wr, wc, sr, sc = bench.dump_selection(16384, 16384)
    nbytes = 8 * 4 * (len(wr) * len(wc) + len(sr) * len(sc)) + 8 * 10000
    assert nbytes < 64 * 2 ** 20, nbytes
    assert len(set(sr)) == len(sr) and sr.max() < 16384 and sc.max() < 16384
    assert np.array_equal(bench.dump_selection(16384, 16384)[2], sr)
