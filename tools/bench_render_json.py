#!/usr/bin/env python3
"""Device and wall time of the JSON and the scalar block of the device renderer
(render_json.render_json / render_scalars, AdminMetricsExportTelemeter.handle_bytes,
PrometheusTelemeter.render_bytes(scalars_on_device=True)) -- a measurement tool, not a test.

The state and the names of bench_render.py: a 2^20-series engine ingests one C3-style Zipf
batch and one le_counts_into call leaves the summaries (and the `le` rows) in device
buffers; names of C5's shape, uploaded once.  --reps rounds in ONE process, every round
running each call once in turn, median (min-max) per call:

  (a) render_json of 2^20 stat rows against render_summaries of the same rows, output in
      device memory: device time by L5DH_PARAM_TIMING, all kernel ids summed
  (b) render_json of 2^20 counter rows, the same way: one lane of a wave's 64 writes a row
  (c) wall time of handle_bytes against handle on a C5-shaped tree (--rows stats, --rows
      counters, --rows / 10 gauges): with the table and the records kept on the device, and
      with nothing kept; the bodies are asserted equal as bytes
  (d) wall time of render_bytes(scalars_on_device=True) against the default on that tree

Bound: (c) device < host.  --mode kernels runs (a) and (b) three times each and nothing else, for
`rocprofv3 --kernel-trace --stats -- python tools/bench_render_json.py --worker --mode
kernels` in a run of its own.  --parent-lib LIB also alternates LIB (a build of the parent
commit) and this build, one fresh process each, A B A B, timing render_summaries and
render_le: the existing blocks must stay within the parent's own min-max range.  Each
worker runs under a time limit; if one fails or runs out of time nothing more is started
on the GPU.  Prints one JSON line (and writes it to --out); exit status 0 when the bound
holds.
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


def worker(args):
    import numpy as np
    import torch

    from linkerd_amd import _native as N
    from linkerd_amd import synth
    from linkerd_amd.engine import QUERY, HistogramEngine
    from linkerd_amd.prometheus import NameTable

    S, R = args.series, args.rows
    dev = torch.device("cuda", args.device)
    eng = HistogramEngine(S, device=args.device)
    eng.set_param(N.PARAM_TIMING, 1)
    series, vals = synth.c3(S=S, N=args.samples, seed=3)
    eng.ingest(torch.from_numpy(series).to(dev), torch.from_numpy(vals).to(dev))
    cuts16, labels16 = HistogramEngine.le_cuts(BOUNDS16)
    d_summ = torch.empty((S * 11,), dtype=torch.int64, device=dev)
    d_le = torch.empty((S, 17), dtype=torch.int64, device=dev)
    d_sums = torch.empty((S,), dtype=torch.int64, device=dev)
    eng.le_counts_into(cuts16, d_le, d_sums, series=d_summ)
    assert int(d_le[:, 16].sum()) == args.samples
    sc = [scope_of(j) for j in range(S)]
    names = NameTable.build([f"rt:client:{STAT}"] * S, [f'rt="{s[1]}", client="{s[3]}"' for s in sc], np.arange(S))
    d_names = names.to_device(args.device)
    out = {"rows_all": S}

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

    out["summaries_bytes"] = eng.render_summaries(d_names, d_summ, out=QUERY)
    out["le_bytes"] = eng.render_le(d_names, d_le, d_sums, labels16, out=QUERY)
    if args.mode == "old":  # what the parent commit's library has too
        d_text = torch.empty((max(out["summaries_bytes"], out["le_bytes"]),), dtype=torch.uint8, device=dev)
        rounds({"summaries_ms": lambda: device_ms(lambda: eng.render_summaries(d_names, d_summ, out=d_text)),
                "le_ms": lambda: device_ms(lambda: eng.render_le(d_names, d_le, d_sums, labels16, out=d_text))}, args.reps)
        eng.close()
        print(json.dumps(out), flush=True)
        return

    from linkerd_amd.admin_metrics import AdminMetricsExportTelemeter, flat_name_table
    from linkerd_amd.prometheus import PrometheusTelemeter, stat_name_table
    from linkerd_amd.render_json import render_json
    from linkerd_amd.telemetry import HistogramSummary, MetricsTree, MetricsTreeStatsReceiver

    # (a), (b): the JSON names of every series (rt/<router>/client/<id>/request_latency_ms), one kind each
    keys = ["/".join(s + (STAT,)) for s in sc]
    j_stats = NameTable.build(keys, [""] * S, np.arange(S), None, np.full(S, N.KIND_STAT, np.uint8)).to_device(args.device)
    j_counters = NameTable.build(keys, [""] * S, np.arange(S), None,
                                 np.full(S, N.KIND_COUNTER, np.uint8)).to_device(args.device)
    d_counters = d_summ.view(S, 11)[:, 3].contiguous()  # the sums: counters of a realistic spread
    out["json_stats_bytes"] = render_json(eng, j_stats, d_summ, None, None, out=QUERY)
    out["json_counters_bytes"] = render_json(eng, j_counters, None, d_counters, None, out=QUERY)
    d_text = torch.empty((max(out["summaries_bytes"], out["json_stats_bytes"]),), dtype=torch.uint8, device=dev)
    device_calls = {
        "json_stats_ms": lambda: device_ms(lambda: render_json(eng, j_stats, d_summ, None, None, out=d_text)),
        "summaries_ms": lambda: device_ms(lambda: eng.render_summaries(d_names, d_summ, out=d_text)),
        "json_counters_ms": lambda: device_ms(lambda: render_json(eng, j_counters, None, d_counters, None, out=d_text)),
    }
    if args.mode == "kernels":
        for _ in range(3):
            for fn in device_calls.values():
                fn()
        eng.close()
        print(json.dumps(out), flush=True)
        return
    rounds(device_calls, args.reps)

    # (c), (d): a C5-shaped tree of R stats (the first R series), R counters, R / 10 gauges
    tree = MetricsTree()
    stats = MetricsTreeStatsReceiver(tree)
    recs = d_summ.view(S, 11)[:R].cpu().numpy().view(N.SUMMARY_DTYPE).reshape(R)
    for j in range(R):
        m = stats.scope(*sc[j]).stat(STAT)
        m.series_id = j
        m._set_snapshot(HistogramSummary.from_record(recs[j]))
        stats.scope(*sc[j]).counter("requests").incr(int(recs[j]["sum"]) + j)
    for g in range(R // 10):
        stats.scope("jvm", f"pool{g}").add_gauge("used", f=lambda g=g: g * 1.5e5 + 0.25)
    d_recs = d_summ[:R * 11].contiguous()
    tel = AdminMetricsExportTelemeter(tree)
    flat = flat_name_table(tree)
    ptel = PrometheusTelemeter(tree)
    d_stat_names = stat_name_table(tree).to_device(args.device)
    uri = "/admin/metrics.json"
    rounds({
        "handle_bytes_device_ms": lambda: wall_ms(lambda: tel.handle_bytes(uri, eng, names=flat, summaries=d_recs))[0],
        "handle_bytes_host_ms": lambda: wall_ms(lambda: tel.handle_bytes(uri, eng))[0],
        "render_bytes_scalars_device_ms": lambda: wall_ms(
            lambda: ptel.render_bytes(eng, names=d_stat_names, summaries=d_recs, scalars_on_device=True))[0],
        "render_bytes_ms": lambda: wall_ms(lambda: ptel.render_bytes(eng, names=d_stat_names, summaries=d_recs))[0],
    }, args.reps)
    python_ms = []
    for _ in range(args.python_reps):
        t, (status, _, text) = wall_ms(lambda: tel.handle(uri))
        python_ms.append(t)
    want = text.encode("utf-8")
    assert status == 200
    assert tel.handle_bytes(uri, eng, names=flat, summaries=d_recs)[2] == want  # the same bytes
    assert tel.handle_bytes(uri, eng)[2] == want
    assert (ptel.render_bytes(eng, names=d_stat_names, summaries=d_recs, scalars_on_device=True) ==
            ptel.render_bytes(eng, names=d_stat_names, summaries=d_recs))
    out.update(rows=R, counters=R, gauges=R // 10, document_bytes=len(want), python_handle_ms=statistics.median(python_ms),
               python_handle_min_max_ms=[min(python_ms), max(python_ms)], python_reps=args.python_reps)
    eng.close()
    print(json.dumps(out), flush=True)


def run_worker(args, mode, lib=None):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--mode", mode]
    for k in ("series", "samples", "rows", "reps", "python_reps", "device"):
        cmd += ["--" + k.replace("_", "-"), str(getattr(args, k))]
    env = dict(os.environ)
    if lib:
        env["L5DH_LIB"] = os.path.abspath(lib)
    try:
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=args.step_timeout, env=env)
    except subprocess.TimeoutExpired:
        sys.exit(f"bench_render_json: a worker ran out of its {args.step_timeout} s; nothing more is started")
    if r.returncode != 0:
        sys.exit(f"bench_render_json: a worker ended with status {r.returncode}; nothing more is started")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--series", type=int, default=1 << 20)
    p.add_argument("--samples", type=int, default=16_000_000, help="samples of the Zipf batch")
    p.add_argument("--rows", type=int, default=100_000, help="stats (and counters; a tenth as many gauges) of the tree")
    p.add_argument("--reps", type=int, default=10, help="timed rounds (median)")
    p.add_argument("--python-reps", type=int, default=3, help="rounds of the Python writer (seconds each)")
    p.add_argument("--device", type=int, default=0)
    p.add_argument("--step-timeout", type=int, default=540, help="seconds for each worker process")
    p.add_argument("--parent-lib", default=None, help="a libl5dhist.so of the parent commit: A/B of the existing blocks")
    p.add_argument("--ab-rounds", type=int, default=3, help="A B pairs of the A/B")
    p.add_argument("--out", default=None, help="also write the JSON line here")
    p.add_argument("--mode", default="new", choices=("new", "old", "kernels"), help=argparse.SUPPRESS)
    p.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    args = p.parse_args()
    if args.worker:
        worker(args)
        return 0
    from linkerd_amd import _native as N
    line = {"tool": "bench_render_json", "series": args.series, "samples": args.samples, "reps": args.reps,
            "date": datetime.date.today().isoformat(), "engine_source_hash": N.engine_source_hash()}
    line.update(run_worker(args, "new"))
    line["json_stats_over_summaries"] = line["json_stats_ms"] / line["summaries_ms"]
    if args.parent_lib:
        keys = ("summaries_ms", "le_ms", "summaries_min_max_ms", "le_min_max_ms")
        ab = {who: {k: [] for k in keys} for who in ("parent", "this")}
        for _ in range(args.ab_rounds):
            for who, lib in (("parent", args.parent_lib), ("this", None)):
                got = run_worker(args, "old", lib)
                for k in keys:
                    ab[who][k].append(got[k])
        line["ab_existing_blocks"] = ab
        # this build's median of the runs' medians against the parent's own slowest call of the session
        line["ab_within_parent_range"] = {
            k + "_ms": bool(statistics.median(ab["this"][k + "_ms"]) <= max(hi for _, hi in ab["parent"][k + "_min_max_ms"]))
            for k in ("summaries", "le")}
    line["accepted"] = bool(line["handle_bytes_device_ms"] < line["python_handle_ms"] and
                            line["handle_bytes_host_ms"] < line["python_handle_ms"])
    text = json.dumps(line)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0 if line["accepted"] else 1


if __name__ == "__main__":
    sys.exit(main())
