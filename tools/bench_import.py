#!/usr/bin/env python3
"""Device time of state import and sparse export (HistogramEngine.import_state /
export_sparse_into / import_sparse) -- a measurement tool, not a test.

The state of bench_le.py / bench_render.py: a 2^20-series engine A ingests one C3-style
Zipf batch (linkerd_amd.synth.c3), folded by a first export.  A second engine B of the same
size receives the imports; a whole-range resetting snapshot makes it clean again (untimed).
--reps rounds in ONE process, every round running each call once in turn, device time by
L5DH_PARAM_TIMING with all kernel ids summed, median (min-max); every buffer is in device
memory:

  (a) A.export_state(reset=False), full range: the yardstick (7.5 GB written)
  (b) B.import_state of (a)'s rows, B clean: the same bytes in the opposite direction
  (c) B.import_state of the same rows once more, B all dirty: the state rows are read as well
  (d) A.export_sparse: the same rows read, a small fraction written
  (e) B.import_sparse of (d), B clean: the touched tiles' rows are written once (zero fill)

Bounds, each against yardsticks of the same process: (b) <= (a) + (a)'s min-max spread,
(c) <= 1.5 (a) + the spread, (d) < (a), (e) <= (b) + the spread.  After the rounds B's dense
rows are compared with A's (both imports, on the device).  The worker runs under a time limit;
if it fails or runs out of time nothing more is started on the GPU.  Prints one JSON line (and
writes it to --out); exit status 0 when every bound holds.
"""
import argparse
import datetime
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)


def worker(args):
    import torch

    from linkerd_amd import _native as N
    from linkerd_amd import synth
    from linkerd_amd.engine import HistogramEngine

    S = args.series
    dev = torch.device("cuda", args.device)
    A, B = HistogramEngine(S, device=args.device), HistogramEngine(S, device=args.device)
    for e in (A, B):
        e.set_param(N.PARAM_TIMING, 1)
    series, vals = synth.c3(S=S, N=args.samples, seed=3)
    A.ingest(torch.from_numpy(series).to(dev), torch.from_numpy(vals).to(dev))
    d_counts = torch.empty((S, N.NBUCKETS), dtype=torch.int32, device=dev)
    d_totals = torch.empty((S,), dtype=torch.int64, device=dev)
    A.export_state(counts=d_counts, totals=d_totals)  # (folds the batch into the state rows)
    n_entries = A.export_sparse_size()
    d_off = torch.empty((S + 1,), dtype=torch.int64, device=dev)
    d_entries = torch.empty((n_entries,), dtype=torch.int64, device=dev)
    d_stot = torch.empty((S,), dtype=torch.int64, device=dev)
    d_summ = torch.empty((S * 11,), dtype=torch.int64, device=dev)
    out = {"series": S, "entries": n_entries, "nonempty_series": int((d_counts != 0).any(dim=1).sum()),
           "dense_bytes": S * (N.NBUCKETS * 4 + 8), "sparse_bytes": n_entries * 8 + (S + 1) * 8 + S * 8}

    def device_ms(eng, fn):
        eng.sync()
        eng.kernel_times(reset=True)
        fn()
        return sum(t for t, _ in eng.kernel_times(reset=True).values())

    def clean_b():
        B.snapshot_into(summaries=d_summ, reset=True)
        assert B.export_sparse_size() == 0

    def import_sparse_clean():
        clean_b()
        return device_ms(B, lambda: B.import_sparse(d_off, d_entries, d_stot))

    def import_dense_clean():
        clean_b()
        return device_ms(B, lambda: B.import_state(d_counts, d_totals))

    calls = {
        "export_state_ms": lambda: device_ms(A, lambda: A.export_state(counts=d_counts, totals=d_totals)),
        "import_state_clean_ms": import_dense_clean,
        "import_state_dirty_ms": lambda: device_ms(B, lambda: B.import_state(d_counts, d_totals)),
        "export_sparse_ms": lambda: device_ms(A, lambda: A.export_sparse_into(d_off, d_entries, d_stot)),
        "import_sparse_clean_ms": import_sparse_clean,
    }
    ms = {k: [] for k in calls}
    for rep in range(args.reps + 1):  # the first round (allocations, code objects) is dropped
        for key, fn in calls.items():
            t = fn()
            if rep:
                ms[key].append(t)
    # what B holds is what A holds: after the last sparse import, and after a dense one
    d_check = torch.empty_like(d_counts)
    d_ctot = torch.empty_like(d_totals)
    B.export_state(counts=d_check, totals=d_ctot)
    out["sparse_import_equal"] = bool(torch.equal(d_check, d_counts) and torch.equal(d_ctot, d_totals))
    import_dense_clean()
    B.export_state(counts=d_check, totals=d_ctot)
    out["dense_import_equal"] = bool(torch.equal(d_check, d_counts) and torch.equal(d_ctot, d_totals))
    for key, v in ms.items():
        out[key] = statistics.median(v)
        out[key.replace("_ms", "_min_max_ms")] = [min(v), max(v)]
    A.close()
    B.close()
    print(json.dumps(out), flush=True)


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--series", type=int, default=1 << 20)
    p.add_argument("--samples", type=int, default=16_000_000, help="samples of the Zipf batch")
    p.add_argument("--reps", type=int, default=10, help="timed rounds (median)")
    p.add_argument("--device", type=int, default=0)
    p.add_argument("--step-timeout", type=int, default=540, help="seconds for the worker process")
    p.add_argument("--out", default=None, help="also write the JSON line here")
    p.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    args = p.parse_args()
    if args.worker:
        worker(args)
        return 0
    from linkerd_amd import _native as N
    line = {"tool": "bench_import", "series": args.series, "samples": args.samples, "reps": args.reps,
            "date": datetime.date.today().isoformat(), "engine_source_hash": N.engine_source_hash()}
    cmd = [sys.executable, os.path.abspath(__file__), "--worker"]
    for k in ("series", "samples", "reps", "device"):
        cmd += ["--" + k, str(getattr(args, k))]
    try:
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=args.step_timeout)
    except subprocess.TimeoutExpired:
        sys.exit(f"bench_import: the worker ran out of its {args.step_timeout} s; nothing more is started")
    if r.returncode != 0:
        sys.exit(f"bench_import: the worker ended with status {r.returncode}; nothing more is started")
    line.update(json.loads(r.stdout.strip().splitlines()[-1]))
    a, (a_min, a_max) = line["export_state_ms"], line["export_state_min_max_ms"]
    spread = a_max - a_min
    line["bounds"] = {
        "b_import_clean_le_a_plus_spread": bool(line["import_state_clean_ms"] <= a + spread),
        "c_import_dirty_le_1.5a_plus_spread": bool(line["import_state_dirty_ms"] <= 1.5 * a + spread),
        "d_export_sparse_lt_a": bool(line["export_sparse_ms"] < a),
        "e_import_sparse_le_b_plus_spread": bool(line["import_sparse_clean_ms"] <= line["import_state_clean_ms"] + spread),
    }
    line["accepted"] = bool(all(line["bounds"].values()) and line["sparse_import_equal"] and line["dense_import_equal"])
    text = json.dumps(line)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0 if line["accepted"] else 1


if __name__ == "__main__":
    sys.exit(main())
