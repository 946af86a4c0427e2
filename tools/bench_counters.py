#!/usr/bin/env python3
"""Counters on the device, measured -- a measurement tool, not a test.

(a) l5dh_counters_add of --adds (2^27) adds from device buffers, device time by
L5DH_PARAM_TIMING (L5DH_K_COUNTERS), --reps rounds in ONE process after a warm-up round,
median (min-max).  Load shapes: Zipf(1.0) over 2^20 counters, Zipf over 10^5 counters, uniform
over 2^20 counters, every add to one id.  The Zipf ranks are scattered over the ids by a fixed
random permutation, so the claim table's home slot (id mod C) is not flattered by rank-ordered
ids.  Each shape under the default variant (the LDS claim table) and under
L5DH_PARAM_VARIANT bit 3 (one global atomic per add), with deltas null and given.  Reported:
adds per second and the LDS share of CounterEngine.info().

The condition for the default: the claim table stays the default only if its median is below
the plain variant's minimum on both Zipf shapes and on the one-id shape (the uniform shape is
exempt: there the table is overhead, which is recorded).

(b) wall time of AdminMetricsExportTelemeter.handle_bytes, ending with the body in host
memory, on a C5-shaped tree (--rows Stats, --rows counters, a tenth as many gauges) with the
table kept and the snapshot's records in device memory: the tree's counters in a CounterEngine
against the same tree with host counters, in the same process, alternating.  Required: the
device-counter median is below the host-counter minimum.  Also recorded: a device-to-host
copy of as many bytes as the body.

Each part runs in a worker under a time limit; if one fails or runs out of time nothing more
is started on the GPU.  Prints one JSON line (and writes it to --out); exit status 0 when both
conditions hold.
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

SHAPES = ("zipf_2p20", "zipf_1e5", "uniform_2p20", "one_id")


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def add_worker(args):
    import numpy as np
    import torch

    from linkerd_amd import _native as N
    from linkerd_amd import synth
    from linkerd_amd.counters import CounterEngine
    from linkerd_amd.engine import HistogramEngine

    dev = torch.device("cuda", args.device)
    n, cap = args.adds, 1 << 20
    eng = HistogramEngine(1024, device=args.device)
    eng.set_param(N.PARAM_TIMING, 1)
    ce = CounterEngine(eng, cap)
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)

    def zipf(k):
        cdf = torch.from_numpy(synth.zipf_cdf(k)).to(dev)
        perm = torch.from_numpy(np.random.default_rng(k).permutation(k).astype(np.int32)).to(dev)
        out = torch.empty((n,), dtype=torch.int32, device=dev)
        step = 1 << 24
        for o in range(0, n, step):
            m = min(step, n - o)
            u = torch.rand((m,), dtype=torch.float64, device=dev, generator=gen)
            rank = torch.searchsorted(cdf, u, right=True).clamp_(max=k - 1)
            out[o:o + m] = perm[rank]
        return out

    def ids_of(shape):
        if shape == "zipf_2p20":
            return zipf(1 << 20)
        if shape == "zipf_1e5":
            return zipf(100_000)
        if shape == "uniform_2p20":
            return torch.randint(0, cap, (n,), dtype=torch.int32, device=dev, generator=gen)
        return torch.full((n,), 12345, dtype=torch.int32, device=dev)

    deltas = torch.randint(-1000, 1000, (n,), dtype=torch.int32, device=dev, generator=gen)
    out = {"adds": n, "counters": cap, "results": {}}
    for shape in SHAPES:
        ids = ids_of(shape)
        torch.cuda.synchronize()
        out["hottest_share_" + shape] = float(torch.bincount(ids[:1 << 22]).max()) / (1 << 22)
        want = None
        for variant, vname in ((0, "table"), (N.VARIANT_COUNTERS_PLAIN, "plain")):
            eng.set_param(N.PARAM_VARIANT, variant)
            for dl, dname in ((None, "null"), (deltas, "given")):
                ce.kernel_time(reset=True)
                ce.add(ids, dl)  # the warm-up round (code objects, allocations) is dropped
                warm = ce.kernel_time(reset=True)[0]
                reps = 3 if warm > args.slow_call_ms else args.reps  # (a call of seconds: fewer rounds, and said so)
                ms = []
                for rep in range(reps):
                    if rep == reps - 1:  # the last round's values are compared across the variants
                        ce.write(0, None)
                    before = ce.info()
                    ce.add(ids, dl)
                    ms.append(ce.kernel_time(reset=True)[0])
                after = ce.info()
                key = f"{shape}/{vname}/deltas_{dname}"
                r = spread(ms)
                r.update(rounds=len(ms), adds_per_s=n / (r["median"] * 1e-3),
                         lds_share=(after["lds_adds"] - before["lds_adds"]) / n)
                out["results"][key] = r
                eng.sync()
                got = ce.device_values().clone()
                torch.cuda.synchronize()
                if variant == 0:
                    want = dict(want or {}, **{dname: got})
                else:
                    r["same_values_as_table"] = bool(torch.equal(got, want[dname]))
                print(key, json.dumps(r), file=sys.stderr, flush=True)
        del ids
    eng.set_param(N.PARAM_VARIANT, 0)
    eng.close()
    print(json.dumps(out), flush=True)


def scrape_worker(args):
    import numpy as np
    import torch

    from linkerd_amd import _native as N
    from linkerd_amd.admin_metrics import AdminMetricsExportTelemeter, flat_name_table
    from linkerd_amd.counters import CounterEngine
    from linkerd_amd.engine import HistogramEngine
    from linkerd_amd.telemetry import HistogramSummary, MetricsTree, MetricsTreeStatsReceiver
    from tools.bench_render import STAT, scope_of

    R = args.rows
    dev = torch.device("cuda", args.device)
    eng = HistogramEngine(max(R, 1024), device=args.device)
    ce = CounterEngine(eng, R)
    rng = np.random.default_rng(5)
    recs = np.zeros(R, N.SUMMARY_DTYPE)
    for f in N.SUMMARY_FIELDS[:-1]:
        recs[f] = rng.integers(1, 1 << 40, R)
    recs["avg"] = recs["sum"] / recs["count"]
    d_recs = torch.from_numpy(recs.view(np.int64).reshape(-1).copy()).to(dev)
    values = rng.integers(0, 1 << 45, R)

    def build(counters):
        tree = MetricsTree(counters=counters)
        stats = MetricsTreeStatsReceiver(tree)
        made = []
        for j in range(R):
            scope = stats.scope(*scope_of(j))
            m = scope.stat(STAT)
            m.series_id = j
            m._set_snapshot(HistogramSummary.from_record(recs[j]))
            made.append(scope.counter("requests"))
        for g in range(R // 10):
            stats.scope("jvm", f"pool{g}").add_gauge("used", f=lambda g=g: g * 1.5e5 + 0.25)
        return tree, made

    host_tree, host_counters = build(None)
    for m, v in zip(host_counters, values.tolist()):
        m.incr(v)
    dev_tree, dev_counters = build(ce)
    ids = np.asarray([m.counter_id for m in dev_counters])
    vals = np.zeros(R, np.int64)
    vals[ids] = values
    ce.write(0, vals)
    tels = {"host": (AdminMetricsExportTelemeter(host_tree), flat_name_table(host_tree)),
            "device": (AdminMetricsExportTelemeter(dev_tree), flat_name_table(dev_tree))}
    uri = "/admin/metrics.json"

    def wall_ms(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        r = fn()
        return (time.perf_counter() - t) * 1e3, r

    ms = {k: [] for k in tels}
    body = {}
    for rep in range(args.reps + 1):  # the first round is dropped
        for who, (tel, flat) in tels.items():
            t, (status, _, text) = wall_ms(lambda: tel.handle_bytes(uri, eng, names=flat, summaries=d_recs))
            assert status == 200
            body[who] = text
            if rep:
                ms[who].append(t)
    assert body["host"] == body["device"], "the two trees print different documents"
    d_text = torch.zeros((len(body["host"]),), dtype=torch.uint8, device=dev)
    copy = [wall_ms(lambda: d_text.cpu())[0] for _ in range(args.reps + 1)][1:]
    out = {"rows": R, "counters": R, "gauges": R // 10, "document_bytes": len(body["host"]),
           "handle_bytes_host_counters_ms": spread(ms["host"]), "handle_bytes_device_counters_ms": spread(ms["device"]),
           "copy_back_ms": spread(copy)}
    eng.close()
    print(json.dumps(out), flush=True)


def run_worker(args, part):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", part]
    for k in ("adds", "rows", "reps", "device", "slow_call_ms"):
        cmd += ["--" + k.replace("_", "-"), str(getattr(args, k))]
    try:
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=args.step_timeout)
    except subprocess.TimeoutExpired:
        sys.exit(f"bench_counters: the {part} worker ran out of its {args.step_timeout} s; nothing more is started")
    if r.returncode != 0:
        sys.exit(f"bench_counters: the {part} worker ended with status {r.returncode}; nothing more is started")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--adds", type=int, default=1 << 27)
    p.add_argument("--rows", type=int, default=100_000, help="Stats (and counters; a tenth as many gauges) of the tree")
    p.add_argument("--reps", type=int, default=8, help="timed rounds (median)")
    p.add_argument("--slow-call-ms", type=float, default=5000.0,
                   help="a configuration whose warm-up call takes longer runs 3 timed rounds only")
    p.add_argument("--device", type=int, default=0)
    p.add_argument("--step-timeout", type=int, default=900, help="seconds for each worker process")
    p.add_argument("--parts", default="add,scrape")
    p.add_argument("--out", default=None, help="also write the JSON line here")
    p.add_argument("--worker", default=None, choices=("add", "scrape"), help=argparse.SUPPRESS)
    args = p.parse_args()
    if args.worker:
        (add_worker if args.worker == "add" else scrape_worker)(args)
        return 0
    from linkerd_amd import _native as N
    line = {"tool": "bench_counters", "reps": args.reps, "date": datetime.date.today().isoformat(),
            "engine_source_hash": N.engine_source_hash()}
    ok = True
    if "add" in args.parts:
        line["add"] = run_worker(args, "add")
        res = line["add"]["results"]
        cond = {}
        for shape in ("zipf_2p20", "zipf_1e5", "one_id"):
            for d in ("null", "given"):
                cond[f"{shape}/deltas_{d}"] = bool(res[f"{shape}/table/deltas_{d}"]["median"] <
                                                   res[f"{shape}/plain/deltas_{d}"]["min"])
        line["table_below_plain_min"] = cond
        line["table_stays_default"] = all(cond.values())
        ok = ok and line["table_stays_default"]
    if "scrape" in args.parts:
        line["scrape"] = run_worker(args, "scrape")
        s = line["scrape"]
        s["device_median_below_host_min"] = bool(s["handle_bytes_device_counters_ms"]["median"] <
                                                 s["handle_bytes_host_counters_ms"]["min"])
        ok = ok and s["device_median_below_host_min"]
    line["accepted"] = bool(ok)
    text = json.dumps(line)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
