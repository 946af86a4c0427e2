#!/usr/bin/env python3
"""Device and wall time of the device renderer (HistogramEngine.render_summaries /
render_le, PrometheusTelemeter.render_bytes) -- a measurement tool, not a test.

The state of bench_le.py: a 2^20-series engine ingests one C3-style Zipf batch
(linkerd_amd.synth.c3), and one le_counts_into call leaves the summaries, the `le` rows at
16 bounds and the sums in device buffers.  Names are synthetic, of C5's shape
(rt/<router>/client/<id>/request_latency_ms), uploaded once.  --reps rounds in ONE
process, every round running each call once in turn, median (min-max) per call:

  (a) render_summaries of all rows, output in device memory: device time by
      L5DH_PARAM_TIMING, all kernel ids summed (length pass, scan, write pass, staging)
  (b) render_le of all rows, the same way
  (c) a device-to-device copy of exactly the bytes (a) and (b) produced (torch events): how
      far the renderer is from just writing the text
  (d) wall time of render_bytes on the first --rows rows (names and records in device
      memory; and with everything on the host), the copy of the text to the host included
  (e) wall time of render() -- the Python exporter -- on the same rows of the same tree

Bound: (d) < (e).  The worker runs under a time limit; if it fails or runs out of time
nothing more is started on the GPU.  Prints one JSON line (and writes it to --out); exit
status 0 when the bound holds.
"""
import argparse
import datetime
import json
import os
import statistics
import subprocess
import sys
import time
import types

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

BOUNDS16 = (1, 2, 5, 10, 25, 50, 100, 250, 500, 1000, 2500, 5000, 10000, 30000, 60000, float("inf"))
STAT = "request_latency_ms"


def scope_of(j):
    return ("rt", f"router{j % 64}", "client", f"$inet$10.{(j >> 16) & 255}.{(j >> 8) & 255}.{j & 255}$8080")


def worker(args):
    import numpy as np
    import torch

    from linkerd_amd import _native as N
    from linkerd_amd import synth
    from linkerd_amd.engine import QUERY, HistogramEngine
    from linkerd_amd.prometheus import NameTable, PrometheusTelemeter, line_multiset, stat_name_table
    from linkerd_amd.telemetry import HistogramSummary, MetricsTree, MetricsTreeStatsReceiver

    S, R = args.series, args.rows
    dev = torch.device("cuda", args.device)
    eng = HistogramEngine(S, device=args.device)
    eng.set_param(N.PARAM_TIMING, 1)
    series, vals = synth.c3(S=S, N=args.samples, seed=3)
    eng.ingest(torch.from_numpy(series).to(dev), torch.from_numpy(vals).to(dev))
    cuts16, labels16 = HistogramEngine.le_cuts(BOUNDS16)
    assert len(cuts16) == 16
    d_summ = torch.empty((S * 11,), dtype=torch.int64, device=dev)
    d_le = torch.empty((S, 17), dtype=torch.int64, device=dev)
    d_sums = torch.empty((S,), dtype=torch.int64, device=dev)
    eng.le_counts_into(cuts16, d_le, d_sums, series=d_summ)
    assert int(d_le[:, 16].sum()) == args.samples

    # names of every series, prepared once and uploaded once
    sc = [scope_of(j) for j in range(S)]
    names = NameTable.build([f"rt:client:{STAT}"] * S, [f'rt="{s[1]}", client="{s[3]}"' for s in sc], np.arange(S))
    d_names = names.to_device(args.device)
    out = {"rows_all": S}
    out["summaries_bytes"] = eng.render_summaries(d_names, d_summ, out=QUERY)
    out["le_bytes"] = eng.render_le(d_names, d_le, d_sums, labels16, out=QUERY)
    big = max(out["summaries_bytes"], out["le_bytes"])
    d_text, d_copy = (torch.empty((big,), dtype=torch.uint8, device=dev) for _ in range(2))

    def copy_ms(nbytes):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        d_copy[:nbytes].copy_(d_text[:nbytes])
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def device_ms(fn):
        eng.sync()
        eng.kernel_times(reset=True)
        fn()
        return sum(t for t, _ in eng.kernel_times(reset=True).values())

    # the first R rows as a tree: what render() walks, and what render_bytes replaces
    tree = MetricsTree()
    stats = MetricsTreeStatsReceiver(tree)
    made = [stats.scope(*sc[j]).stat(STAT) for j in range(R)]
    recs = d_summ.view(S, 11)[:R].cpu().numpy().view(N.SUMMARY_DTYPE).reshape(R)
    for j, m in enumerate(made):
        m.series_id = j
        m._set_snapshot(HistogramSummary.from_record(recs[j]))
    h_host = types.SimpleNamespace(le_cuts=cuts16, le_labels=labels16, le_buckets=d_le[:R].cpu().numpy().view(np.uint64),
                                   le_sums=d_sums[:R].cpu().numpy())
    h_dev = types.SimpleNamespace(le_cuts=cuts16, le_labels=labels16, le_buckets=d_le[:R].contiguous(),
                                  le_sums=d_sums[:R].contiguous())
    tree_names = stat_name_table(tree)
    assert tree_names.index.tolist() == [m.series_id for m in tree_names.metrics]
    d_tree_names = tree_names.to_device(args.device)
    d_recs = d_summ[:R * 11].contiguous()
    tel_host, tel_dev = PrometheusTelemeter(tree, histograms=h_host), PrometheusTelemeter(tree, histograms=h_dev)

    def wall_ms(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        r = fn()
        return (time.perf_counter() - t) * 1e3, r

    calls = {
        "summaries_ms": lambda: device_ms(lambda: eng.render_summaries(d_names, d_summ, out=d_text)),
        "copy_summaries_ms": lambda: copy_ms(out["summaries_bytes"]),
        "le_ms": lambda: device_ms(lambda: eng.render_le(d_names, d_le, d_sums, labels16, out=d_text)),
        "copy_le_ms": lambda: copy_ms(out["le_bytes"]),
        "render_bytes_device_ms": lambda: wall_ms(lambda: tel_dev.render_bytes(eng, names=d_tree_names, summaries=d_recs))[0],
        "render_bytes_host_ms": lambda: wall_ms(lambda: tel_host.render_bytes(eng, names=tree_names))[0],
    }
    ms = {k: [] for k in calls}
    for rep in range(args.reps + 1):  # the first round (allocations, code objects) is dropped
        for key, fn in calls.items():
            t = fn()
            if rep:
                ms[key].append(t)
    python_ms = []
    for _ in range(args.python_reps):
        t, text = wall_ms(tel_host.render)
        python_ms.append(t)
    # the texts are the same text
    want = line_multiset(text)
    assert line_multiset(tel_dev.render_bytes(eng, names=d_tree_names, summaries=d_recs).decode()) == want
    assert line_multiset(tel_host.render_bytes(eng, names=tree_names).decode()) == want
    for key, v in ms.items():
        out[key] = statistics.median(v)
        out[key.replace("_ms", "_min_max_ms")] = [min(v), max(v)]
    out.update(rows=R, rows_bytes=len(text.encode()), python_render_ms=statistics.median(python_ms),
               python_render_min_max_ms=[min(python_ms), max(python_ms)], python_reps=args.python_reps)
    eng.close()
    print(json.dumps(out), flush=True)


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--series", type=int, default=1 << 20)
    p.add_argument("--samples", type=int, default=16_000_000, help="samples of the Zipf batch")
    p.add_argument("--rows", type=int, default=100_000, help="rows of the tree render() and render_bytes print")
    p.add_argument("--reps", type=int, default=10, help="timed rounds (median)")
    p.add_argument("--python-reps", type=int, default=3, help="rounds of the Python exporter (seconds each)")
    p.add_argument("--device", type=int, default=0)
    p.add_argument("--step-timeout", type=int, default=540, help="seconds for the worker process")
    p.add_argument("--out", default=None, help="also write the JSON line here")
    p.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    args = p.parse_args()
    if args.worker:
        worker(args)
        return 0
    from linkerd_amd import _native as N
    line = {"tool": "bench_render", "series": args.series, "samples": args.samples, "reps": args.reps,
            "date": datetime.date.today().isoformat(), "engine_source_hash": N.engine_source_hash()}
    cmd = [sys.executable, os.path.abspath(__file__), "--worker"]
    for k in ("series", "samples", "rows", "reps", "python_reps", "device"):
        cmd += ["--" + k.replace("_", "-"), str(getattr(args, k))]
    try:
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=args.step_timeout)
    except subprocess.TimeoutExpired:
        sys.exit(f"bench_render: the worker ran out of its {args.step_timeout} s; nothing more is started")
    if r.returncode != 0:
        sys.exit(f"bench_render: the worker ended with status {r.returncode}; nothing more is started")
    line.update(json.loads(r.stdout.strip().splitlines()[-1]))
    line["summaries_over_copy"] = line["summaries_ms"] / line["copy_summaries_ms"]
    line["le_over_copy"] = line["le_ms"] / line["copy_le_ms"]
    line["accepted"] = bool(line["render_bytes_device_ms"] < line["python_render_ms"] and
                            line["render_bytes_host_ms"] < line["python_render_ms"])
    text = json.dumps(line)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0 if line["accepted"] else 1


if __name__ == "__main__":
    sys.exit(main())
