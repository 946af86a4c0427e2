#!/usr/bin/env python3
"""Device and wall time of the InfluxDB body of the device renderer
(render_influx.render_influx, InfluxDbTelemeter.render_bytes) -- a measurement tool, not a
test.

The state of bench_render_json.py: a 2^20-series engine ingests one C3-style Zipf batch and
one le_counts_into call leaves the summaries in a device buffer.  One process, a warm-up
round, then --reps rounds running each call once in turn; median (min-max) per call:

  (a) render_influx over the fields of 2^20 Stats (11 * 2^20 rows, a line per Stat, names
      of C5's shape), table, values and output in device memory: device time by
      L5DH_PARAM_TIMING, all kernel ids summed -- beside a device-to-device copy of the
      same number of bytes, timed by events
  (b) wall time, ending with the text in host memory, on a C5-shaped tree (--rows stats,
      --rows counters, --rows / 10 gauges): render_bytes with the table kept and the
      records in device memory, render_bytes with nothing kept, and InfluxDbTelemeter.render,
      the existing writer; the bodies are asserted equal as bytes

Bound: (b) the kept-table form is faster than render in every round.  --mode kernels runs
(a) three times and nothing else, for `rocprofv3 --kernel-trace --stats -- python
tools/bench_render_influx.py --worker --mode kernels` in a run of its own.  The worker runs
under a time limit; if it fails or runs out of time nothing more is started on the GPU.
Prints one JSON line (and writes it to --out); exit status 0 when the bound holds.
"""
import argparse
import datetime
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tools.bench_render import BOUNDS16, STAT, scope_of  # noqa: E402


def stat_fields_table(S):
    """The table influx_table builds for S Stats each alone under its client scope, put
    together from arrays (a tree of 2^20 Stats takes minutes to walk): a line per Stat, its
    eleven fields in key order, index the series id."""
    import numpy as np

    from linkerd_amd import _native as N
    from linkerd_amd.render_influx import STAT_FIELDS, InfluxTable, pack_texts
    fields = sorted(STAT_FIELDS)  # (ASCII suffixes: the UTF-16 order)
    keys = [(STAT + sfx).encode() for sfx, _ in fields]
    klen = np.asarray([len(k) for k in keys], np.uint64)
    key_off = np.zeros(11 * S + 1, np.uint64)
    key_off[1:] = np.cumsum(np.tile(klen, S))
    key_bytes = np.tile(np.frombuffer(b"".join(keys), np.uint8), S)
    sc = [scope_of(j) for j in range(S)]
    head_off, head_bytes = pack_texts([f"rt:client,client={s[3]},host=" for s in sc])
    tail_off, tail_bytes = pack_texts([f",rt={s[1]} " for s in sc])
    series = np.repeat(np.arange(S, dtype=np.uint32), 11)
    return InfluxTable(series.copy(), np.full(11 * S, N.KIND_STAT, np.uint8),
                       np.tile(np.asarray([f for _, f in fields], np.uint8), S), series, key_off, key_bytes, head_off,
                       head_bytes, tail_off, tail_bytes)


def worker(args):
    import numpy as np
    import torch

    from linkerd_amd import _native as N
    from linkerd_amd import synth
    from linkerd_amd.engine import QUERY, HistogramEngine
    from linkerd_amd.influxdb import InfluxDbTelemeter
    from linkerd_amd.render_influx import influx_table, render_influx
    from linkerd_amd.telemetry import HistogramSummary, MetricsTree, MetricsTreeStatsReceiver

    S, R = args.series, args.rows
    dev = torch.device("cuda", args.device)
    eng = HistogramEngine(S, device=args.device)
    eng.set_param(N.PARAM_TIMING, 1)
    series, vals = synth.c3(S=S, N=args.samples, seed=3)
    eng.ingest(torch.from_numpy(series).to(dev), torch.from_numpy(vals).to(dev))
    cuts16, _ = HistogramEngine.le_cuts(BOUNDS16)
    d_summ = torch.empty((S * 11,), dtype=torch.int64, device=dev)
    d_le = torch.empty((S, 17), dtype=torch.int64, device=dev)
    d_sums = torch.empty((S,), dtype=torch.int64, device=dev)
    eng.le_counts_into(cuts16, d_le, d_sums, series=d_summ)
    assert int(d_le[:, 16].sum()) == args.samples
    del d_le, d_sums
    out = {"stats_all": S, "rows_all": 11 * S}

    def device_ms(fn):
        eng.sync()
        eng.kernel_times(reset=True)
        fn()
        return sum(t for t, _ in eng.kernel_times(reset=True).values())

    def wall_ms(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        r = fn()
        return (time.perf_counter() - t) * 1e3, r

    def rounds(calls, reps):
        ms = {k: [] for k in calls}
        for rep in range(reps + 1):  # the first round (allocations, code objects) is dropped
            for key, fn in calls.items():
                t = fn()
                if rep:
                    ms[key].append(t)
        for key, v in ms.items():
            out[key] = statistics.median(v)
            out[key.replace("_ms", "_min_max_ms")] = [min(v), max(v)]

    # (a) the fields of every series, everything on the device
    host_all = stat_fields_table(S)
    d_all = host_all.to_device(args.device)
    nbytes = out["influx_bytes"] = render_influx(eng, d_all, "none", d_summ, None, None, out=QUERY)
    d_text = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    d_copy = torch.empty((nbytes,), dtype=torch.uint8, device=dev)

    def copy_ms():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        d_copy.copy_(d_text)
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    device_calls = {"influx_ms": lambda: device_ms(lambda: render_influx(eng, d_all, "none", d_summ, None, None, out=d_text)),
                    "copy_ms": copy_ms}
    if args.mode == "kernels":
        for _ in range(3):
            device_calls["influx_ms"]()
        eng.close()
        print(json.dumps(out), flush=True)
        return
    rounds(device_calls, args.reps)
    # the same bytes as the Python replay prints for the first Stats' lines
    first = 64
    want = render_influx(eng, host_all.take(np.arange(11 * first)), "none", d_summ, None, None)
    assert d_text[:len(want)].cpu().numpy().tobytes() == want and want.count(b"\n") == first
    del d_all, d_text, d_copy, host_all
    torch.cuda.empty_cache()

    # (b) a C5-shaped tree of R stats (the first R series), R counters, R / 10 gauges
    tree = MetricsTree()
    stats = MetricsTreeStatsReceiver(tree)
    recs = d_summ.view(S, 11)[:R].cpu().numpy().view(N.SUMMARY_DTYPE).reshape(R)
    for j in range(R):
        sc = stats.scope(*scope_of(j))
        m = sc.stat(STAT)
        m.series_id = j
        m._set_snapshot(HistogramSummary.from_record(recs[j]))
        sc.counter("requests").incr(int(recs[j]["sum"]) + j)
    for g in range(R // 10):
        stats.scope("jvm", f"pool{g}").add_gauge("used", f=lambda g=g: g * 1.5e5 + 0.25)
    d_recs = d_summ[:R * 11].contiguous()
    tel = InfluxDbTelemeter(tree)
    tel.render("none")  # (the tree's first walk orders every node's children once: no call below pays for that)
    t0 = time.perf_counter()
    table = influx_table(tree)
    out["influx_table_ms"] = (time.perf_counter() - t0) * 1e3
    rounds({"render_bytes_kept_ms": lambda: wall_ms(lambda: tel.render_bytes(eng, "none", table=table, summaries=d_recs))[0],
            "render_bytes_ms": lambda: wall_ms(lambda: tel.render_bytes(eng, "none"))[0]}, args.reps)
    python_ms = []
    for _ in range(args.python_reps):
        t, text = wall_ms(lambda: tel.render("none"))
        python_ms.append(t)
    want = text.encode("utf-8")
    assert tel.render_bytes(eng, "none", table=table, summaries=d_recs) == want  # the same bytes
    assert tel.render_bytes(eng, "none") == want
    out.update(rows=R, counters=R, gauges=R // 10, field_rows=table.n, lines=table.nlines, body_bytes=len(want),
               python_render_ms=statistics.median(python_ms), python_render_min_max_ms=[min(python_ms), max(python_ms)],
               python_reps=args.python_reps)
    eng.close()
    print(json.dumps(out), flush=True)


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--series", type=int, default=1 << 20)
    p.add_argument("--samples", type=int, default=16_000_000, help="samples of the Zipf batch")
    p.add_argument("--rows", type=int, default=100_000, help="stats (and counters; a tenth as many gauges) of the tree")
    p.add_argument("--reps", type=int, default=8, help="timed rounds (median)")
    p.add_argument("--python-reps", type=int, default=3, help="rounds of the Python writer (seconds each)")
    p.add_argument("--device", type=int, default=0)
    p.add_argument("--step-timeout", type=int, default=540, help="seconds for the worker process")
    p.add_argument("--out", default=None, help="also write the JSON line here")
    p.add_argument("--mode", default="all", choices=("all", "kernels"), help=argparse.SUPPRESS)
    p.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    args = p.parse_args()
    if args.worker:
        worker(args)
        return 0
    from linkerd_amd import _native as N
    line = {"tool": "bench_render_influx", "series": args.series, "samples": args.samples, "reps": args.reps,
            "date": datetime.date.today().isoformat(), "engine_source_hash": N.engine_source_hash()}
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--mode", "all"]
    for k in ("series", "samples", "rows", "reps", "python_reps", "device"):
        cmd += ["--" + k.replace("_", "-"), str(getattr(args, k))]
    try:
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=args.step_timeout)
    except subprocess.TimeoutExpired:
        sys.exit(f"bench_render_influx: the worker ran out of its {args.step_timeout} s; nothing more is started")
    if r.returncode != 0:
        sys.exit(f"bench_render_influx: the worker ended with status {r.returncode}; nothing more is started")
    line.update(json.loads(r.stdout.strip().splitlines()[-1]))
    line["influx_over_copy"] = line["influx_ms"] / line["copy_ms"]
    line["influx_gb_per_s"] = line["influx_bytes"] / line["influx_ms"] / 1e6
    line["python_over_kept"] = line["python_render_ms"] / line["render_bytes_kept_ms"]
    line["python_over_nothing_kept"] = line["python_render_ms"] / line["render_bytes_ms"]
    # the kept-table form against the writer: its slowest round against the writer's fastest
    line["accepted"] = bool(line["render_bytes_kept_min_max_ms"][1] < line["python_render_min_max_ms"][0])
    text = json.dumps(line)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0 if line["accepted"] else 1


if __name__ == "__main__":
    sys.exit(main())
