#!/usr/bin/env python3
"""Device time of the configurable quantiles (HistogramEngine.quantiles*) against calls of
the same library that read the same rows -- a measurement tool, not a test.

A 2^20-series engine ingests one C3-style Zipf batch (linkerd_amd.synth.c3) and takes a
non-resetting full snapshot, so every tile is dirty and folded; the dense rows of the same
state are exported once into device buffers.  Then, device time by L5DH_PARAM_TIMING (all
kernel ids summed), --reps rounds in ONE process, every round running each call once in
turn (so a drift of the machine falls on all of them alike), median and min-max per call:

  (a) summarize_dense of the device rows: the yardstick -- it reads the same 7192 B per
      row, resolves 8 targets per row and writes 88 B per row
  (b) quantiles(reset=False), K = 16, of the live state (128 B per row written)
  (c) quantiles_dense, K = 16, of the device rows
  (d) quantiles(reset=False), K = 64 (512 B per row written: 0.5 GB): reported, not bound
  (e) le_counts(reset=False) at 16 bounds of the live state: the sibling query, reported
  (f) render_quantiles, K = 16, of all rows into device memory: bytes and ms, reported

Bound: (b) and (c) <= median(a) + (max(a) - min(a)).  The worker runs under a time limit;
if it fails or runs out of time nothing more is started on the GPU.  Prints one JSON line
(and writes it to --out); exit status 0 when the bound holds.
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

BOUNDS16 = (1, 2, 5, 10, 25, 50, 100, 250, 500, 1000, 2500, 5000, 10000, 30000, 60000, float("inf"))
Q16 = (0.01, 0.05, 0.1, 0.25, 0.3, 0.4, 0.6, 0.7, 0.75, 0.8, 0.85, 0.975, 0.995, 0.9995, 0.99995, 0.999999)


def worker(args):
    import numpy as np
    import torch

    from linkerd_amd import _native as N
    from linkerd_amd import synth
    from linkerd_amd.engine import QUERY, HistogramEngine
    from linkerd_amd.prometheus import NameTable

    S = args.series
    eng = HistogramEngine(S, device=args.device)
    eng.set_param(N.PARAM_TIMING, 1)
    series, vals = synth.c3(S=S, N=args.samples, seed=3)
    dev = torch.device("cuda", args.device)
    eng.ingest(torch.from_numpy(series).to(dev), torch.from_numpy(vals).to(dev))
    summ = eng.snapshot(reset=False)  # folds every pending record into the state rows
    assert int(summ["count"].sum()) == args.samples
    out = {"dirty_series": int((summ["count"] > 0).sum())}
    cuts16, _ = HistogramEngine.le_cuts(BOUNDS16)
    q16 = np.array(Q16, np.float64)
    q64 = (np.arange(64, dtype=np.float64) + 0.5) / 64.0
    assert len(cuts16) == 16 and q16.size == 16
    d_counts = torch.empty((S, N.NBUCKETS), dtype=torch.int32, device=dev)
    d_totals = torch.empty((S,), dtype=torch.int64, device=dev)
    d_summ = torch.empty((S * 11,), dtype=torch.int64, device=dev)
    d_q16 = torch.empty((S, 16), dtype=torch.int64, device=dev)
    d_q16d = torch.empty((S, 16), dtype=torch.int64, device=dev)
    d_q64 = torch.empty((S, 64), dtype=torch.int64, device=dev)
    d_le16 = torch.empty((S, 17), dtype=torch.int64, device=dev)
    d_sums = torch.empty((S,), dtype=torch.int64, device=dev)
    eng.export_state(reset=False, counts=d_counts, totals=d_totals)
    # names of every series, prepared once and uploaded once (tools/bench_render.py's)
    names = NameTable.build(["rt:client:request_latency_ms"] * S,
                            [f'rt="router{j % 64}", client="$inet$10.{(j >> 16) & 255}.{(j >> 8) & 255}.{j & 255}$8080"'
                             for j in range(S)], np.arange(S))
    d_names = names.to_device(args.device)
    eng.quantiles_into(q16, d_q16)
    out["render_bytes"] = eng.render_quantiles(d_names, d_q16, q16, out=QUERY)
    d_text = torch.empty((out["render_bytes"],), dtype=torch.uint8, device=dev)
    calls = {
        "summarize_dense_ms": lambda: eng.summarize_dense(d_counts, d_totals, d_summ),
        "quantiles_live_k16_ms": lambda: eng.quantiles_into(q16, d_q16),
        "quantiles_dense_k16_ms": lambda: eng.quantiles_into(q16, d_q16d, dense=d_counts),
        "quantiles_live_k64_ms": lambda: eng.quantiles_into(q64, d_q64),
        "le_live_k16_ms": lambda: eng.le_counts_into(cuts16, d_le16, d_sums),
        "render_quantiles_k16_ms": lambda: eng.render_quantiles(d_names, d_q16, q16, out=d_text),
    }
    ms = {k: [] for k in calls}
    for rep in range(args.reps + 1):  # the first round (allocations, code objects) is dropped
        for key, fn in calls.items():
            eng.sync()
            eng.kernel_times(reset=True)
            fn()
            t = sum(t for t, _ in eng.kernel_times(reset=True).values())
            if rep:
                ms[key].append(t)
    # live and dense agree, the median column is the summary's p50, every sample was counted
    assert torch.equal(d_q16, d_q16d)
    assert bool((d_q64[:, 1:] >= d_q64[:, :-1]).all())  # (quantiles ascend with q)
    p50 = np.array([0.5])
    d_p50 = torch.empty((S, 1), dtype=torch.int64, device=dev)
    eng.quantiles_into(p50, d_p50)
    assert torch.equal(d_p50[:, 0], d_summ.view(S, 11)[:, 4])
    assert int(d_le16[:, 16].sum()) == args.samples and int(d_summ.view(S, 11)[:, 0].sum()) == args.samples
    for key, v in ms.items():
        out[key] = statistics.median(v)
        out[key.replace("_ms", "_min_max_ms")] = [min(v), max(v)]
    eng.close()
    print(json.dumps(out), flush=True)


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--series", type=int, default=1 << 20)
    p.add_argument("--samples", type=int, default=16_000_000, help="samples of the Zipf batch")
    p.add_argument("--reps", type=int, default=10, help="timed rounds (median; >= 10)")
    p.add_argument("--device", type=int, default=0)
    p.add_argument("--step-timeout", type=int, default=400, help="seconds for the worker process")
    p.add_argument("--out", default=None, help="also write the JSON line here")
    p.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    args = p.parse_args()
    if args.worker:
        worker(args)
        return 0
    if args.reps < 10:
        p.error("--reps must be at least 10")
    from linkerd_amd import _native as N
    line = {"tool": "bench_quantiles", "series": args.series, "samples": args.samples, "reps": args.reps,
            "date": datetime.date.today().isoformat(), "engine_source_hash": N.engine_source_hash()}
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--series", str(args.series),
           "--samples", str(args.samples), "--reps", str(args.reps), "--device", str(args.device)]
    try:
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=args.step_timeout)
    except subprocess.TimeoutExpired:
        sys.exit(f"bench_quantiles: the worker ran out of its {args.step_timeout} s; nothing more is started")
    if r.returncode != 0:
        sys.exit(f"bench_quantiles: the worker ended with status {r.returncode}; nothing more is started")
    line.update(json.loads(r.stdout.strip().splitlines()[-1]))
    lo, hi = line["summarize_dense_min_max_ms"]
    line["bound_ms"] = line["summarize_dense_ms"] + (hi - lo)
    line["live_ok"] = bool(line["quantiles_live_k16_ms"] <= line["bound_ms"])
    line["dense_ok"] = bool(line["quantiles_dense_k16_ms"] <= line["bound_ms"])
    line["k64_over_k16"] = line["quantiles_live_k64_ms"] / line["quantiles_live_k16_ms"]
    line["accepted"] = line["live_ok"] and line["dense_ok"]
    text = json.dumps(line)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0 if line["accepted"] else 1


if __name__ == "__main__":
    sys.exit(main())
