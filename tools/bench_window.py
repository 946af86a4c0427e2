#!/usr/bin/env python3
"""Device time of a sliding-window query (window.Window.summaries_into) beside what a caller
had to do without it -- a measurement tool, not a test.

The state of bench_render.py / bench_import.py: a 2^20-series engine A; six intervals, each
one C3-style Zipf batch (linkerd_amd.synth.c3, consecutive sample indices), are ingested and
pushed into a ring of six slots.  Before each push the interval's sparse rows are also
exported to device buffers: the CSR rows a caller would have had to keep.  --reps rounds in
ONE process after a warm-up round, every round running each call once in turn, device time
by L5DH_PARAM_TIMING with all kernel ids summed, median (min-max); every buffer is in device
memory:

  (w) A's window: summaries_into(last = 6), summaries of all 2^20 series
  (x) the alternative: six import_sparse of the same rows into a second engine B of the same
      size (7.5 GB of dense state) and B.snapshot with summaries (reset=False); B is cleaned
      by a resetting snapshot outside the timing
  (c) a device copy of as many bytes as (w) reads and writes (torch, timed by events)

Acceptance: (w)'s median is below (x)'s median, and both wrote the same summaries.  Also
recorded: the ring's bytes, the entries per slot, (w)'s bytes per ms.  The worker runs under a
time limit; if it fails or runs out of time nothing more is started on the GPU.  Prints one
JSON line (and writes it to --out); exit status 0 when accepted.
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

INTERVALS = 6


def worker(args):
    import torch

    from linkerd_amd import _native as N
    from linkerd_amd import synth
    from linkerd_amd.engine import HistogramEngine
    from linkerd_amd.window import Window

    S = args.series
    dev = torch.device("cuda", args.device)
    A, B = HistogramEngine(S, device=args.device), HistogramEngine(S, device=args.device)
    for e in (A, B):
        e.set_param(N.PARAM_TIMING, 1)
    win = Window(A, INTERVALS)
    cdf = synth.zipf_cdf(S)
    csr, per_slot = [], []
    for i in range(INTERVALS):
        series, vals = synth.c3(S=S, N=args.samples, seed=3, base_index=i * args.samples, cdf=cdf)
        A.ingest(torch.from_numpy(series).to(dev), torch.from_numpy(vals).to(dev))
        n = A.export_sparse_size()  # (folds the batch into the state rows)
        d_off = torch.empty((S + 1,), dtype=torch.int64, device=dev)
        d_entries = torch.empty((max(n, 1),), dtype=torch.int64, device=dev)
        d_tot = torch.empty((S,), dtype=torch.int64, device=dev)
        assert A.export_sparse_into(d_off, d_entries, d_tot) == n
        csr.append((d_off, d_entries, d_tot))
        per_slot.append(n)
        win.push()
    info = win.info()
    assert info["filled"] == INTERVALS and info["entries"] == sum(per_slot)
    d_w = torch.zeros((S * 11,), dtype=torch.int64, device=dev)
    d_x = torch.zeros((S * 11,), dtype=torch.int64, device=dev)
    d_scratch = torch.zeros((S * 11,), dtype=torch.int64, device=dev)
    # what the query moves: the entries, two offsets and a total per slot and series, the forget
    # marks; the summaries out
    moved = 8 * sum(per_slot) + INTERVALS * S * 24 + 8 * S + 88 * S
    out = {"series": S, "intervals": INTERVALS, "entries_per_slot": per_slot, "ring_bytes": info["bytes"],
           "dense_state_bytes": S * (1800 * 4 + 16), "query_bytes": moved}

    def device_ms(eng, fn):
        eng.sync()
        eng.kernel_times(reset=True)
        eng.kernel_time(N.K_WINDOW, reset=True)
        fn()
        return sum(t for t, _ in eng.kernel_times(reset=True).values()) + eng.kernel_time(N.K_WINDOW, reset=True)[0]

    def alternative():
        for d_off, d_entries, d_tot in csr:
            B.import_sparse(d_off, d_entries, d_tot)
        B.snapshot_into(summaries=d_x, reset=False)

    def alternative_ms():
        t = device_ms(B, alternative)
        B.snapshot_into(summaries=d_scratch, reset=True)  # (clean again, untimed)
        return t

    src = torch.empty((moved,), dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)

    def copy_ms():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        dst.copy_(src)
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    calls = {"window_ms": lambda: device_ms(A, lambda: win.summaries_into(INTERVALS, d_w)),
             "alternative_ms": alternative_ms, "copy_ms": copy_ms}
    ms = {k: [] for k in calls}
    for rep in range(args.reps + 1):  # the first round (allocations, code objects) is dropped
        for key, fn in calls.items():
            t = fn()
            if rep:
                ms[key].append(t)
    out["same_summaries"] = bool(torch.equal(d_w, d_x))
    out["series_with_samples"] = int((d_w.view(S, 11)[:, 0] != 0).sum())
    for key, v in ms.items():
        out[key] = statistics.median(v)
        out[key.replace("_ms", "_min_max_ms")] = [min(v), max(v)]
    out["query_bytes_per_ms"] = moved / out["window_ms"]
    out["copy_bytes_per_ms"] = moved / out["copy_ms"]
    A.close()
    B.close()
    print(json.dumps(out), flush=True)


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--series", type=int, default=1 << 20)
    p.add_argument("--samples", type=int, default=16_000_000, help="samples of each interval's Zipf batch")
    p.add_argument("--reps", type=int, default=8, help="timed rounds (median)")
    p.add_argument("--device", type=int, default=0)
    p.add_argument("--step-timeout", type=int, default=540, help="seconds for the worker process")
    p.add_argument("--out", default=None, help="also write the JSON line here")
    p.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    args = p.parse_args()
    if args.worker:
        worker(args)
        return 0
    from linkerd_amd import _native as N
    line = {"tool": "bench_window", "series": args.series, "samples": args.samples, "reps": args.reps,
            "date": datetime.date.today().isoformat(), "engine_source_hash": N.engine_source_hash()}
    cmd = [sys.executable, os.path.abspath(__file__), "--worker"]
    for k in ("series", "samples", "reps", "device"):
        cmd += ["--" + k, str(getattr(args, k))]
    try:
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=args.step_timeout)
    except subprocess.TimeoutExpired:
        sys.exit(f"bench_window: the worker ran out of its {args.step_timeout} s; nothing more is started")
    if r.returncode != 0:
        sys.exit(f"bench_window: the worker ended with status {r.returncode}; nothing more is started")
    line.update(json.loads(r.stdout.strip().splitlines()[-1]))
    line["accepted"] = bool(line["window_ms"] < line["alternative_ms"] and line["same_summaries"])
    text = json.dumps(line)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0 if line["accepted"] else 1


if __name__ == "__main__":
    sys.exit(main())
