"""bench.py's command line: a plain run times the steps and prints the result line,
`--full` adds the check, the per-kernel figures and the CPU baseline, and
`--dump-outputs DIR` writes what the last timed step returned -- the same arrays in
every run with the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, N = 3001, 300_000  # more series than a counts dump keeps whole, not a multiple of the 32-series tile
ARGS = ["--gpus", "1", "--series", str(S), "--samples", str(N), "--steps", "2", "--warmup", "1"]
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def _bench(*args):
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), *args],
                       capture_output=True, text=True, timeout=240, cwd=REPO)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d)) if f.endswith(".npy")}


def test_dump_rows_are_fixed_and_the_largest_dump_fits():
    sys.path.insert(0, REPO)
    import bench
    assert np.array_equal(bench.dump_rows(100, 2048, 1), np.arange(100))
    a, b = bench.dump_rows(1_000_000, 2048, 2), bench.dump_rows(1_000_000, 2048, 2)
    assert np.array_equal(a, b) and a.size == 2048 and np.unique(a).size == 2048
    assert np.array_equal(a[:bench.DUMP_HEAD_ROWS], np.arange(bench.DUMP_HEAD_ROWS)) and a.max() < 1_000_000
    # C3 (1M series): series_counts + summary rows + bucket_totals + counts rows + the two row lists
    total = 8 * (1_000_000 + bench.DUMP_SUMMARY_ROWS * 12 + 1798 + bench.DUMP_COUNT_ROWS * 1799)
    assert total <= 64_000_000


def test_steps_below_one_are_rejected():
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--dry-run", "--steps", "0"],
                       capture_output=True, text=True, timeout=240, cwd=REPO)
    assert r.returncode == 2 and "--steps" in r.stderr


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("plain"))
    return _bench(*ARGS, "--dump-outputs", d), _load(d)


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_the_last_step(plain):
    line, out = plain
    assert all(k in line for k in HEADLINE)
    assert line["steps"] == 2 and line["ms_per_step"] > 0 and line["full"] is False
    # (ms_per_step is printed to 1e-4 ms)
    assert line["value"] == pytest.approx(N / (line["ms_per_step"] * 1e-3), rel=1e-4 / line["ms_per_step"] + 1e-6)
    assert line["kernels"] is None and line["roofline"] is None and line["cpu_baseline"] is None
    assert set(out) == {"series_counts", "summary", "summary_rows", "bucket_totals", "counts", "counts_rows"}
    assert all(a.dtype == np.float64 for a in out.values())
    assert out["series_counts"].shape == (S,) and out["series_counts"].sum() == N
    assert out["bucket_totals"].shape == (1798,) and out["bucket_totals"].sum() == N
    assert out["summary"].shape == (S, 11) and np.array_equal(out["summary_rows"], np.arange(S))
    assert np.array_equal(out["summary"][:, 0], out["series_counts"])
    rows = out["counts_rows"].astype(np.int64)
    assert out["counts"].shape == (rows.size, 1798) and rows.size < S
    assert np.array_equal(out["counts"].sum(axis=1), out["series_counts"][rows])


@pytest.mark.gpu
def test_full_run_adds_its_figures_and_computes_the_same(plain, tmp_path):
    line = _bench(*ARGS, "--full", "--cpu-threads", "2", "--dump-outputs", str(tmp_path))
    assert all(k in line for k in HEADLINE) and line["full"] is True and line["steps"] == 2
    assert line["kernels"] and all("avg_ms" in k for k in line["kernels"].values())
    priced = {"bin1", "accum"} & set(line["kernels"])  # the phases bench.KERNEL_ALG_BYTES prices
    assert (line["roofline"] is not None) == bool(priced)
    assert line["cpu_baseline"]["value"] > 0
    out = _load(str(tmp_path))
    assert set(out) == set(plain[1])
    for name, a in plain[1].items():
        assert np.array_equal(out[name], a), name
