#!/usr/bin/env python3
"""Device time of label rollups (HistogramEngine.rollup) against the dense export of
the same state -- a measurement tool, not a test.

A 2^20-series engine ingests one C3-style Zipf batch (linkerd_amd.synth.c3) and takes a
non-resetting full snapshot, so every tile is dirty and folded.  Then, device time by
L5DH_PARAM_TIMING (all kernel ids summed), median of --reps calls each:

  (a) export_state(reset=False) of the full range into device buffers: the yardstick --
      it reads the same rows as a rollup and also writes as many bytes
  (b) rollup(reset=False), 1024 interleaved groups (i % 1024)
  (c) rollup(reset=False), 1024 contiguous groups (i // 1024)
  (d) rollup(reset=False), every series in one group
  (e) rollup(with_series=True, reset=True) after a fresh batch, against
      snapshot(reset=True) after the same batch

(a)-(d) run in one worker process and (e) in a second one, each under its own time
limit; a worker that fails or runs out of time ends the run (nothing more is started
on the GPU).  Prints one JSON line (and writes it to --out); exit status 0 when (b)
and (c) took no longer than (a).
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


def _setup(args):
    import numpy as np
    import torch

    from linkerd_amd import _native as N
    from linkerd_amd import synth
    from linkerd_amd.engine import HistogramEngine

    S = args.series
    eng = HistogramEngine(S, device=args.device)
    eng.set_param(N.PARAM_TIMING, 1)
    series, vals = synth.c3(S=S, N=args.samples, seed=3)
    dev = torch.device("cuda", args.device)
    d_series = torch.from_numpy(series).to(dev)
    d_vals = torch.from_numpy(vals).to(dev)
    torch.cuda.synchronize(dev)
    return np, torch, N, eng, dev, d_series, d_vals


def _device_ms(eng, fn, reps, before=None):
    """Median device time of fn() over reps calls (before(): untimed preparation)."""
    ms = []
    for _ in range(reps + 1):  # the first call (allocations) is dropped
        if before is not None:
            before()
        eng.sync()
        eng.kernel_times(reset=True)
        fn()
        ms.append(sum(t for t, _ in eng.kernel_times(reset=True).values()))
    return statistics.median(ms[1:])


def worker_steady(args):
    np, torch, N, eng, dev, d_series, d_vals = _setup(args)
    S, G = args.series, 1024
    eng.ingest(d_series, d_vals)
    summ = eng.snapshot(reset=False)  # folds every pending record into the state rows
    assert int(summ["count"].sum()) == args.samples
    dirty_series = int((summ["count"] > 0).sum())
    del summ
    out = {"dirty_series": dirty_series}
    d_counts = torch.empty((S, N.NBUCKETS), dtype=torch.int32, device=dev)
    d_totals = torch.empty((S,), dtype=torch.int64, device=dev)
    out["export_state_ms"] = _device_ms(
        eng, lambda: eng.export_state(reset=False, counts=d_counts, totals=d_totals), args.reps)
    del d_counts, d_totals
    torch.cuda.empty_cache()
    i = np.arange(S, dtype=np.int64)
    on_dev = lambda m: torch.from_numpy(m.astype(np.uint32)).to(dev)  # noqa: E731
    maps = {"rollup_interleaved_ms": (on_dev(i % G), G),
            "rollup_contiguous_ms": (on_dev(np.minimum(i // max(1, S // G), G - 1)), G),
            "rollup_one_group_ms": (on_dev(np.zeros(S, np.int64)), 1)}
    for key, (gmap, ng) in maps.items():
        o_summ = torch.empty((ng * 11,), dtype=torch.int64, device=dev)
        o_counts = torch.empty((ng, N.NBUCKETS), dtype=torch.int32, device=dev)
        o_totals = torch.empty((ng,), dtype=torch.int64, device=dev)
        out[key] = _device_ms(eng, lambda: eng.rollup_into(gmap, ng, o_summ, o_counts, o_totals), args.reps)
        assert int(o_summ.view(ng, 11)[:, 0].sum()) == args.samples, key  # every sample in exactly one group
    eng.close()
    print(json.dumps(out), flush=True)


def worker_fresh(args):
    np, torch, N, eng, dev, d_series, d_vals = _setup(args)
    S, G = args.series, 1024
    gmap = torch.from_numpy((np.arange(S, dtype=np.int64) % G).astype(np.uint32)).to(dev)
    o_summ = torch.empty((G * 11,), dtype=torch.int64, device=dev)
    o_series = torch.empty((S * 11,), dtype=torch.int64, device=dev)
    fresh = lambda: eng.ingest(d_series, d_vals)  # noqa: E731
    out = {}
    out["rollup_series_reset_ms"] = _device_ms(
        eng, lambda: eng.rollup_into(gmap, G, o_summ, series=o_series, reset=True), args.reps, before=fresh)
    assert int(o_summ.view(G, 11)[:, 0].sum()) == args.samples
    out["snapshot_reset_ms"] = _device_ms(eng, lambda: eng.snapshot_into(o_series, reset=True), args.reps, before=fresh)
    eng.close()
    print(json.dumps(out), flush=True)


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--series", type=int, default=1 << 20)
    p.add_argument("--samples", type=int, default=16_000_000, help="samples of the Zipf batch")
    p.add_argument("--reps", type=int, default=10, help="timed calls per figure (median; >= 10)")
    p.add_argument("--device", type=int, default=0)
    p.add_argument("--step-timeout", type=int, default=240, help="seconds per worker process")
    p.add_argument("--out", default=None, help="also write the JSON line here")
    p.add_argument("--worker", choices=["steady", "fresh"], default=None, help=argparse.SUPPRESS)
    args = p.parse_args()
    if args.worker:
        {"steady": worker_steady, "fresh": worker_fresh}[args.worker](args)
        return 0
    if args.reps < 10:
        p.error("--reps must be at least 10")
    from linkerd_amd import _native as N
    line = {"tool": "bench_rollup", "series": args.series, "samples": args.samples, "reps": args.reps,
            "date": datetime.date.today().isoformat(), "engine_source_hash": N.engine_source_hash()}
    for step in ("steady", "fresh"):
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", step, "--series", str(args.series),
               "--samples", str(args.samples), "--reps", str(args.reps), "--device", str(args.device)]
        try:
            r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=args.step_timeout)
        except subprocess.TimeoutExpired:
            sys.exit(f"bench_rollup: step {step} ran out of its {args.step_timeout} s; nothing more is started")
        if r.returncode != 0:
            sys.exit(f"bench_rollup: step {step} ended with status {r.returncode}; nothing more is started")
        line.update(json.loads(r.stdout.strip().splitlines()[-1]))
    a = line["export_state_ms"]
    line["accepted"] = bool(line["rollup_interleaved_ms"] <= a and line["rollup_contiguous_ms"] <= a)
    text = json.dumps(line)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0 if line["accepted"] else 1


if __name__ == "__main__":
    sys.exit(main())
