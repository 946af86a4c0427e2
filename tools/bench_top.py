#!/usr/bin/env python3
"""Device time of the exact top-k (HistogramEngine.top*) against what a host-side ranking
pays before it can start -- a measurement tool, not a test.

A 2^20-series engine ingests one C3-style Zipf batch (linkerd_amd.synth.c3) and takes a
non-resetting full snapshot, so every tile is dirty and folded.  Then, device time by
L5DH_PARAM_TIMING (all kernel ids summed), --reps rounds in ONE process, every round running
each call once in turn (so a drift of the machine falls on all of them alike), median and
min-max per call:

  (a) snapshot_into (summaries only, device buffer, reset=False): the yardstick of the live call
  (b) top_summaries of (a)'s device buffer, by p99, k = 100, outputs in device memory
  (c) (b) at k = 1024
  (d) top(by="p99", k=100, reset=False), live
  (e) top(by=0.995, k=100, reset=False), live (adds the K = 1 quantile pass)
  (q) quantiles(K = 1, q = 0.995, reset=False): what (e) may add to (d)
  (f) the copy of (a)'s 92 MB buffer into pinned host memory (l5dh_pin_alloc), torch events
  (g) torch.topk over a contiguous int64 copy of the p99 column, k = 100, torch events: for the
      record only, no bound

Bounds, inside this one process: (b) < (f) and (c) < (f); (d) <= (a) + (b) + (a)'s spread;
(e) <= (d) + (q) + (a)'s spread.  After the rounds (b)'s ids must equal a host sorted() of the
copied summaries, and (d)'s ids must equal (b)'s.  The worker runs under a time limit; if it
fails or runs out of time nothing more is started on the GPU.  Prints one JSON line (and
writes it to --out); exit status 0 when the bounds hold.
"""
import argparse
import ctypes
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
    eng.ingest(torch.from_numpy(series).to(dev), torch.from_numpy(vals).to(dev))
    summ = eng.snapshot(reset=False)  # folds every pending record into the state rows
    assert int(summ["count"].sum()) == args.samples
    out = {"dirty_series": int((summ["count"] > 0).sum()), "summary_bytes": S * 88}

    def outputs(k, with_q=False):
        return (torch.zeros(k, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev),
                torch.zeros(k * 11, dtype=torch.int64, device=dev),
                torch.zeros(k, dtype=torch.int64, device=dev) if with_q else None)

    d_summ = torch.empty((S * 11,), dtype=torch.int64, device=dev)
    b_ids, b_n, b_top, _ = outputs(100)
    c_ids, c_n, c_top, _ = outputs(1024)
    d_ids, d_n, d_top, _ = outputs(100)
    e_ids, e_n, e_top, e_q = outputs(100, with_q=True)
    d_q1 = torch.empty((S, 1), dtype=torch.int64, device=dev)
    q1 = np.array([0.995])
    # the pinned host buffer a host-side ranking copies the summaries into
    pin = ctypes.c_void_p()
    assert eng._lib.l5dh_pin_alloc(S * 88, ctypes.byref(pin)) == 0
    h_words = np.ctypeslib.as_array((ctypes.c_int64 * (S * 11)).from_address(pin.value))
    h_summ = torch.from_numpy(h_words)
    d_p99 = torch.empty((S,), dtype=torch.int64, device=dev)
    topk = {}

    def engine_ms(fn):
        eng.sync()
        eng.kernel_times(reset=True)
        fn()
        return sum(t for t, _ in eng.kernel_times(reset=True).values())

    def torch_ms(fn):
        eng.sync()
        torch.cuda.synchronize(dev)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def run_topk():
        topk["values"], topk["ids"] = torch.topk(d_p99, 100)

    calls = {
        "snapshot_ms": lambda: engine_ms(lambda: eng.snapshot_into(d_summ, reset=False)),
        "top_summaries_k100_ms": lambda: engine_ms(lambda: eng.top_into(100, "p99", b_ids, b_n, b_top, values=d_summ)),
        "top_summaries_k1024_ms": lambda: engine_ms(lambda: eng.top_into(1024, "p99", c_ids, c_n, c_top, values=d_summ)),
        "top_live_k100_ms": lambda: engine_ms(lambda: eng.top_into(100, "p99", d_ids, d_n, d_top, reset=False)),
        "top_live_q_k100_ms": lambda: engine_ms(lambda: eng.top_into(100, 0.995, e_ids, e_n, e_top, e_q, reset=False)),
        "quantiles_k1_ms": lambda: engine_ms(lambda: eng.quantiles_into(q1, d_q1)),
        "copy_to_pinned_ms": lambda: torch_ms(lambda: h_summ.copy_(d_summ, non_blocking=True)),
        "torch_topk_k100_ms": lambda: torch_ms(run_topk),
    }
    ms = {k: [] for k in calls}
    for rep in range(args.reps + 1):  # the first round (allocations, code objects) is dropped
        for key, fn in calls.items():
            if key == "torch_topk_k100_ms":  # (its input, outside the timed region)
                d_p99.copy_(d_summ.view(S, 11)[:, 7])
            t = fn()
            if rep:
                ms[key].append(t)
    torch.cuda.synchronize(dev)
    # (b)'s ids against a host sorted() of the copied summaries; (d)'s ids against (b)'s
    host = h_words.view(N.SUMMARY_DTYPE)
    assert host.tobytes() == summ.tobytes()
    p99, cnt = host["p99"].tolist(), host["count"].tolist()
    want = sorted((i for i in range(S) if cnt[i] >= 1), key=lambda i: (-p99[i], i))
    nb, nc = int(b_n.cpu()[0]), int(c_n.cpu()[0])
    assert nb == 100 and nc == 1024
    got_b = b_ids.cpu().numpy().view(np.uint32)
    assert got_b.tolist() == want[:100], "top_summaries differs from the host ranking"
    assert c_ids.cpu().numpy().view(np.uint32).tolist() == want[:1024]
    assert d_ids.cpu().numpy().view(np.uint32).tolist() == got_b.tolist(), "the live ranking differs"
    assert b_top.cpu().numpy().tobytes() == host[got_b].tobytes() == d_top.cpu().numpy().tobytes()
    qv = d_q1.cpu().numpy()[:, 0].tolist()
    want_q = sorted((i for i in range(S) if cnt[i] >= 1), key=lambda i: (-qv[i], i))[:100]
    assert e_ids.cpu().numpy().view(np.uint32).tolist() == want_q and e_q.cpu().numpy().tolist() == [qv[i] for i in want_q]
    assert sorted(topk["values"].cpu().tolist(), reverse=True) == [p99[i] for i in want[:100]]
    for key, v in ms.items():
        out[key] = statistics.median(v)
        out[key.replace("_ms", "_min_max_ms")] = [min(v), max(v)]
    del h_summ, host, h_words
    eng._lib.l5dh_pin_free(pin)
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
    line = {"tool": "bench_top", "series": args.series, "samples": args.samples, "reps": args.reps,
            "date": datetime.date.today().isoformat(), "engine_source_hash": N.engine_source_hash()}
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--series", str(args.series),
           "--samples", str(args.samples), "--reps", str(args.reps), "--device", str(args.device)]
    try:
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=args.step_timeout)
    except subprocess.TimeoutExpired:
        sys.exit(f"bench_top: the worker ran out of its {args.step_timeout} s; nothing more is started")
    if r.returncode != 0:
        sys.exit(f"bench_top: the worker ended with status {r.returncode}; nothing more is started")
    line.update(json.loads(r.stdout.strip().splitlines()[-1]))
    lo, hi = line["snapshot_min_max_ms"]
    spread = hi - lo
    line["k100_below_copy"] = bool(line["top_summaries_k100_ms"] < line["copy_to_pinned_ms"])
    line["k1024_below_copy"] = bool(line["top_summaries_k1024_ms"] < line["copy_to_pinned_ms"])
    line["live_bound_ms"] = line["snapshot_ms"] + line["top_summaries_k100_ms"] + spread
    line["live_ok"] = bool(line["top_live_k100_ms"] <= line["live_bound_ms"])
    line["live_q_bound_ms"] = line["top_live_k100_ms"] + line["quantiles_k1_ms"] + spread
    line["live_q_ok"] = bool(line["top_live_q_k100_ms"] <= line["live_q_bound_ms"])
    line["accepted"] = all(line[k] for k in ("k100_below_copy", "k1024_below_copy", "live_ok", "live_q_ok"))
    text = json.dumps(line)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0 if line["accepted"] else 1


if __name__ == "__main__":
    sys.exit(main())
