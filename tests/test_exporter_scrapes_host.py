"""The Python exporter layer against its parent, byte for byte (no GPU): for a fixed corpus
of trees, every host text (Prometheus, /admin/metrics.json, InfluxDB), every array of every
table the device renderers read, the exact ``l5dh_render_*`` calls of every scrape entry
point as a recording library sees them, the host writers' bytes behind an ERANGE, and what
the snapshot drivers set and return over a fake StatEngine.

The expected records (tests/golden/exporter_scrapes.json) were written by this module's
``__main__`` from the exporter modules of the commit before they were given one labelled
walk, one table module and one scrape selection, and are never written again from a later
one: they pin what those modules did, copy by copy.  To keep the file small, a named tree's
records are stored in full up to 600 characters of JSON, 250 for a call trace (arrays as
dtype, shape and hex bytes, or beyond 32 bytes as ``#length:crc32``); a longer record, and
each whole section of a random tree, is stored as the length and zlib.crc32 of its
canonical JSON text.
"""
import ctypes
import dataclasses
import errno
import json
import os
import zlib
from types import SimpleNamespace
from urllib.parse import quote

import numpy as np
import pytest

from linkerd_amd import _native as N
from linkerd_amd import admin_metrics, influxdb, prometheus, render_influx, rollup, telemetry
from linkerd_amd.telemetry import HistogramSummary, Metric, MetricsTree, MetricsTreeStatsReceiver

from . import influx_cases
from .test_engine_calls_host import RecordingLib, _p, _ref, _v, _w, stub_engine
from .test_fmt_host import exporters_tree

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "exporter_scrapes.json")
CAP = 64  # series of the engines behind the corpus (a tree has at most 40 metrics)
N_RANDOM = 40


# ---- the corpus ----------------------------------------------------------------------------------
def escape_tree():
    """Label values with a backslash, a quote and a newline, under two of the rewrites."""
    tree = MetricsTree()
    stats = MetricsTreeStatsReceiver(tree)
    stats.scope("rt", 'a\\b"c\nd').stat("latency_ms")._set_snapshot(influx_cases.ONE_TWO)
    stats.scope("rt", 'a\\b"c\nd', "client", 'x"\n\\y').counter("requests").incr(5)
    stats.scope("rt", 'a\\b"c\nd', "client", 'x"\n\\y').stat("latency_ms")._set_snapshot(influx_cases.TWO_FOUR)
    return tree


def two_level_tree():
    """Lines at two depths: InfluxDB prints the deeper one first."""
    tree = MetricsTree()
    stats = MetricsTreeStatsReceiver(tree)
    stats.scope("a").counter("c").incr(1)
    stats.scope("a", "b").counter("d").incr(2)
    stats.scope("a", "b").stat("s")._set_snapshot(influx_cases.ONE_TWO)
    return tree


NAMED = dict(influx_cases.NAMED, exporters=lambda: exporters_tree()[0], escape=escape_tree, two_level=two_level_tree)
CORPUS = dict(NAMED, **{f"random_{seed}": (lambda seed=seed: influx_cases.random_tree(seed)) for seed in range(N_RANDOM)})


def build(name):
    """The tree ``name``, its Stats given series ids by counting in walk order; every Stat
    whose count is 3 mod 7 stays without one (the pruned case)."""
    tree = CORPUS[name]()
    count = 0
    for _, t in tree.walk():
        if isinstance(t.metric, Metric.Stat):
            t.metric.series_id = None if count % 7 == 3 else count
            count += 1
    return tree


def side_engine():
    """The attributes the ``le``, quantile and rollup writers read, as seeded arrays."""
    rng = np.random.default_rng(7)
    buckets = np.cumsum(rng.integers(0, 1000, (CAP, 4)), axis=1).astype(np.uint64)
    return SimpleNamespace(capacity=CAP, le_cuts=np.array([3, 9, 20], np.uint32), le_labels=np.array([10, 100, 1000], np.int64),
                           le_buckets=buckets, le_sums=rng.integers(-2 ** 40, 2 ** 40, CAP).astype(np.int64),
                           quantile_q=np.array([0.25, 0.995]), quantile_labels=["0.25", "0.995"],
                           quantile_values=rng.integers(0, 2 ** 31, (CAP, 2)).astype(np.int64))


def records(seed, n=CAP):
    """Seeded summary records (finite avg: every text is inside the formatters' domain)."""
    rng = np.random.default_rng(100 + seed)
    a = np.zeros(n, N.SUMMARY_DTYPE)
    for f in N.SUMMARY_FIELDS:
        a[f] = rng.integers(0, 2 ** 40, n) if f != "avg" else rng.integers(0, 2 ** 20, n) / 8.0
    a["count"][::5] = 0
    return a


# ---- recording -----------------------------------------------------------------------------------
class RenderLib(RecordingLib):
    """RecordingLib plus the three whole-scrape entry points."""

    def _values(self, sp, ns, cp, nc, gp, ng):
        # (gauges as their bits: NaN compares equal to itself)
        return [_w(sp, ctypes.c_int64, 11 * ns), _v(ns), _w(cp, ctypes.c_int64, nc), _v(nc), _w(gp, ctypes.c_uint32, ng),
                _v(ng)]

    def l5dh_render_json(self, ctx, names, kp, n, sp, ns, cp, nc, gp, ng, op, cap, ln):
        rc = self._rec("l5dh_render_json", _v(ctx), self._names(names, n), _w(kp, ctypes.c_uint8, n), _v(n),
                       *self._values(sp, ns, cp, nc, gp, ng), _p(op), _v(cap), _ref(ln))
        return self._text(rc, op, cap, ln)

    def l5dh_render_scalars(self, ctx, names, kp, n, cp, nc, gp, ng, op, cap, ln):
        rc = self._rec("l5dh_render_scalars", _v(ctx), self._names(names, n), _w(kp, ctypes.c_uint8, n), _v(n),
                       *self._values(None, 0, cp, nc, gp, ng)[2:], _p(op), _v(cap), _ref(ln))
        return self._text(rc, op, cap, ln)

    def l5dh_render_influx(self, ctx, names, n, nl, hb, nh, sp, ns, cp, nc, gp, ng, op, cap, ln):
        nm = names._obj
        assert isinstance(nm, N.InfluxNames)
        offs = [_w(getattr(nm, f), ctypes.c_uint64, k + 1) for f, k in (("key_off", n), ("head_off", nl), ("tail_off", nl))]
        table = [_ref(names), _w(nm.line, ctypes.c_uint32, n), _w(nm.kinds, ctypes.c_uint8, n),
                 _w(nm.field, ctypes.c_uint8, n), _w(nm.index, ctypes.c_uint32, n)]
        for off, f in zip(offs, ("key_bytes", "head_bytes", "tail_bytes")):
            table += [off, _w(getattr(nm, f), ctypes.c_uint8, off[-1])]
        rc = self._rec("l5dh_render_influx", _v(ctx), table, _v(n), _v(nl), _w(hb, ctypes.c_uint8, nh), _v(nh),
                       *self._values(sp, ns, cp, nc, gp, ng), _p(op), _v(cap), _ref(ln))
        return self._text(rc, op, cap, ln)


def _short(data: bytes):
    return "#%d:%08x" % (len(data), zlib.crc32(data))


def _plain(x):
    """A record as JSON holds it: arrays as dtype, shape and bytes; in a call trace the
    words behind a pointer, more than 16 of them as length and checksum."""
    if isinstance(x, np.ndarray):
        data = np.ascontiguousarray(x).tobytes()
        return f"{x.dtype}{list(x.shape)}:" + (data.hex() if len(data) <= 32 else _short(data))
    if isinstance(x, bytes):
        return {"utf8": _plain(x.decode("utf-8"))}
    if isinstance(x, str) and len(x) > 300:
        return _short(x.encode("utf-8"))
    if isinstance(x, HistogramSummary):
        return list(dataclasses.astuple(x))
    if isinstance(x, (list, tuple)):
        if len(x) > 17 and isinstance(x[0], str) and x[0] == "ptr" and all(isinstance(w, int) for w in x[1:]):
            return ["ptr", _short(json.dumps(list(x[1:])).encode())]
        return [_plain(v) for v in x]
    if isinstance(x, dict):
        return {str(k): _plain(v) for k, v in x.items()}
    if isinstance(x, (np.integer, np.bool_)):
        return int(x)
    if isinstance(x, np.floating):
        return float(x)
    assert x is None or isinstance(x, (str, int, float)), type(x)
    return x


def scrape(call, **lib_options):
    """One scrape on a fresh stub engine: what came back (or the exception) and the
    ``l5dh_render_*`` calls the library saw, in order."""
    lib = RenderLib(**lib_options)
    e = stub_engine(max_series=CAP, lib=lib)
    e._order_after_torch = lambda: None
    try:
        out = {"result": call(e), "error": None}
    except Exception as ex:  # noqa: BLE001 -- the class is what is recorded
        out = {"result": None, "error": [type(ex).__name__, str(ex)]}
    e._ctx = ctypes.c_void_p()  # (nothing to close)
    out["calls"] = [c for c in lib.calls if c[0].startswith("l5dh_render_")]
    return out


class FakeStatEngine:
    """What the snapshot drivers ask of a StatEngine, answered with seeded records."""

    capacity = CAP

    def __init__(self):
        self.calls = []

    def snapshot_all(self, reset=True):
        self.calls.append(["snapshot_all", reset])
        return records(1)

    def window_summaries(self, last, include_open=False):
        self.calls.append(["window_summaries", last, include_open])
        return records(2)

    def snapshot_all_rollup(self, group_of, ngroups, reset=True):
        self.calls.append(["snapshot_all_rollup", np.asarray(group_of), ngroups, reset])
        return records(3), records(4, ngroups)

    def top(self, k, by, order="largest", min_count=1, group=None, g=0):
        self.calls.append(["top", k, by, order, min_count, None if group is None else np.asarray(group), g])
        ids = np.array([5, 2, 63, 0, 1], np.uint32)[:k]  # (63: no Stat of the corpus holds it)
        res = (ids, records(5, ids.size))
        return res + (np.arange(ids.size, dtype=np.int64) + 1000,) if isinstance(by, float) else res


def _subtree_query(tree):
    """A ``q`` that names a subtree where the tree has one whose name needs no quoting of ``/``."""
    names = list(tree.children)
    return quote(next((n for n in names if "/" not in n), names[0] if names else "none"), safe="")


def _table_arrays(t):
    return {k: v for k, v in vars(t).items() if isinstance(v, np.ndarray) or v is None and k in ("index", "kinds")}


def trace(name):
    """Everything recorded of the tree ``name``: section -> record name -> record."""
    tree = build(name)
    side = side_engine()
    plan = rollup.plan_rollup(tree, ("client",), CAP)
    group_summaries = [influx_cases.SUMMARIES[g % len(influx_cases.SUMMARIES)] for g in range(plan.ngroups)]
    given = records(0)
    q = _subtree_query(tree)
    uris = {"flat": "/admin/metrics.json", "pretty": "/admin/metrics.json?pretty=1", "tree": "/admin/metrics.json?tree=1",
            "subtree": "/admin/metrics.json?q=" + q, "unknown": "/admin/metrics.json?q=no/such"}
    prom = prometheus.PrometheusTelemeter(tree)
    prom_all = prometheus.PrometheusTelemeter(tree, (plan, group_summaries), side, side)
    admin = admin_metrics.AdminMetricsExportTelemeter(tree, engine=None)
    influx = influxdb.InfluxDbTelemeter(tree)
    scalar_lines = []
    prometheus.write_scalar_metrics(tree, scalar_lines)

    out = {"texts": {"prometheus": prom.render(), "prometheus_all": prom_all.render(), "scalars": "".join(scalar_lines)}}
    out["texts"].update({"admin_" + k: list(admin.handle(uri)) for k, uri in uris.items()})
    out["texts"].update({"influx_" + host: influx.render(host) for host in influx_cases.HOSTS})
    out["texts"]["plan"] = {"group_of": plan.group_of, "groups": [[key, [list(kv) for kv in labels]]
                                                                  for key, labels in plan.groups]}

    tables = {"stat_name_table": prometheus.stat_name_table(tree), "scalar_name_table": prometheus.scalar_name_table(tree),
              "rollup_name_table": prometheus.rollup_name_table(plan), "flat_name_table": admin_metrics.flat_name_table(tree),
              "influx_table": render_influx.influx_table(tree)}
    out["tables"] = {}
    for k, t in tables.items():
        out["tables"][k] = _table_arrays(t)
        out["tables"][k + "_take"] = _table_arrays(t.take(range(0, t.n, 2)))

    calls = out["calls"] = {}
    for kept in (False, True):
        for summ in (None, given):
            tag = ("kept" if kept else "built") + ("_given" if summ is not None else "_own")
            names = tables["stat_name_table"] if kept else None
            for on_device in (False, True):
                calls[f"prometheus_{tag}_{'device' if on_device else 'host'}_scalars"] = scrape(
                    lambda e: prom_all.render_bytes(e, names, summ, scalars_on_device=on_device))
            flat = tables["flat_name_table"] if kept else None
            for k in ("flat", "subtree", "pretty"):
                calls[f"admin_{k}_{tag}"] = scrape(lambda e: list(admin.handle_bytes(uris[k], e, flat, summ)))
            table = tables["influx_table"] if kept else None
            calls[f"influx_{tag}"] = scrape(lambda e: influx.render_bytes(e, "h:80", table, summ))
    calls["prometheus_plain"] = scrape(lambda e: prom.render_bytes(e))

    for code, word in ((-errno.ERANGE, "erange"), (-errno.EINVAL, "einval")):
        calls["admin_" + word] = scrape(lambda e: list(admin.handle_bytes(uris["flat"], e)), fail={"l5dh_render_json": code})
        calls["influx_" + word] = scrape(lambda e: influx.render_bytes(e, "none"), fail={"l5dh_render_influx": code})

    out["engine"] = engine_trace(name)
    return _plain(out)


def engine_trace(name):
    """What the snapshot drivers set and return over a FakeStatEngine (a tree of its own:
    they overwrite the snapshots)."""
    tree = build(name)
    path_of = {t.metric: "/".join(p) for p, t in tree.walk() if isinstance(t.metric, Metric.Stat)}

    def snapshots():
        return [[p, m.snapshotted_summary] for m, p in path_of.items()]

    out = {}
    fake = FakeStatEngine()
    out["window_stats"] = [[path_of[m], s] for m, s in telemetry.window_stats(tree, fake, 3, include_open=True).items()]
    scope = tuple(next(iter(tree.children), "none").split("/"))[:1]
    out["top_stats"] = telemetry.top_stats(tree, fake, 4, by="p99")
    out["top_stats_scope"] = telemetry.top_stats(tree, fake, 5, by=0.995, order="smallest", scope=scope)
    out["top_stats_min_count_0"] = telemetry.top_stats(tree, fake, 3, by="avg", min_count=0)
    out["snapshots_before"] = snapshots()
    out["snapshot_histograms"] = telemetry.snapshot_histograms(tree, fake)
    out["snapshots_after"] = snapshots()
    plan = rollup.plan_rollup(tree, ("client",), CAP)
    out["snapshot_histograms_rollup"] = rollup.snapshot_histograms_rollup(tree, fake, plan)
    out["snapshots_after_rollup"] = snapshots()
    out["engine_calls"] = fake.calls
    return out


def stored(name, tr):
    """A trace as the golden file holds it: a named tree in full, of a random tree each
    record as the length and checksum of its canonical JSON text."""
    if name not in NAMED:
        return {section: {"all": _short(json.dumps(recs, sort_keys=True, separators=(",", ":")).encode())}
                for section, recs in tr.items()}
    out = {}
    for section, recs in tr.items():  # (a record equal to an earlier one of its section is stored as that one's name)
        first, out[section] = {}, {}
        for k, rec in recs.items():
            text = json.dumps(rec, sort_keys=True)
            if text in first:
                out[section][k] = {"same_as": first[text]}
            elif len(text) > (250 if section == "calls" else 600):  # (a long one: its checksum; of a trace the renders too)
                brief = {"renders": " ".join(c[0][len("l5dh_render_"):] for c in rec["calls"])} if section == "calls" else {}
                out[section][k] = dict(brief, all=_short(text.encode()))
            else:
                out[section][k] = rec
            first.setdefault(text, k)
    return out


def mismatches(name, want):
    """The records of tree ``name`` that differ from the golden ones, as section/record."""
    got = json.loads(json.dumps(stored(name, trace(name))))
    bad = [f"{s}: records {sorted(set(got.get(s, {})) ^ set(want[s]))}" for s in want if set(got.get(s, {})) != set(want[s])]
    return bad + [f"{s}/{k}" for s in want for k in want[s] if k in got.get(s, {}) and got[s][k] != want[s][k]]


# ---- the tests -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_corpus_is_the_golden_files(golden):
    assert list(golden) == list(CORPUS)
    sections = {"texts", "tables", "calls", "engine"}
    assert all(set(tr) == sections and all(tr[s] for s in sections) for tr in golden.values())


@pytest.mark.parametrize("name", list(CORPUS))
def test_tree_scrapes_as_under_the_parent(golden, name):
    assert mismatches(name, golden[name]) == []


def test_every_render_entry_point_is_reached():
    seen = {c[0] for n in ("root", "exporters") for rec in trace(n)["calls"].values() for c in rec["calls"]}
    assert seen == {n for n in N.SIGNATURES if n.startswith("l5dh_render_")}


# ---- the pin bites: one defect at a time, patched into the code under test ----------------------------
@pytest.fixture
def nametable():
    """The shared module (imported here: the modules the golden file was written from had none)."""
    from linkerd_amd import nametable
    return nametable


def _everywhere(monkeypatch, nametable, name, value):
    """``name`` replaced in the shared module and in every exporter module that imported it."""
    for module in (nametable, prometheus, admin_metrics, influxdb, render_influx, rollup):
        if hasattr(module, name):
            monkeypatch.setattr(module, name, value)


def test_a_rewrite_without_its_label_exists_guard_is_reported(monkeypatch, golden, nametable):
    real = nametable.rewrite

    def unguarded(prefix, labels):
        head, added = real(prefix, ())
        return head, labels + added
    assert ("rt", "r", "service", "s", "service", "t") == influx_cases.TAGGED_TWICE
    _everywhere(monkeypatch, nametable, "rewrite", unguarded)
    bad = mismatches("rewrite", golden["rewrite"])
    assert {"texts/prometheus", "texts/influx_none", "tables/scalar_name_table", "tables/influx_table",
            "calls/influx_built_own", "calls/prometheus_built_own_device_scalars"} <= set(bad), bad


def test_influx_lines_emitted_pre_order_are_reported(monkeypatch, golden, nametable):
    real = nametable.walk
    monkeypatch.setattr(influxdb, "walk", lambda *a, post=False, **kw: real(*a, **kw))
    bad = mismatches("two_level", golden["two_level"])
    assert {"texts/influx_" + host for host in influx_cases.HOSTS} <= set(bad), bad


def test_scalar_ordinals_counted_across_kinds_are_reported(monkeypatch, golden, nametable):
    def across(index, kinds):
        rows = kinds != N.KIND_STAT
        index[rows] = np.arange(int(rows.sum()))
        return index
    _everywhere(monkeypatch, nametable, "scalar_ordinals", across)
    bad = mismatches("root", golden["root"])
    assert {"tables/scalar_name_table", "tables/flat_name_table", "tables/influx_table", "calls/admin_flat_built_own",
            "calls/influx_built_own", "calls/prometheus_built_own_device_scalars"} <= set(bad), bad


if __name__ == "__main__":
    # Writes the expected records.  Only ever run against the exporter modules the records
    # pin (see the module docstring); later ones are compared with the file, not written to it.
    with open(GOLDEN, "w") as f:  # one record per line
        f.write("{" + ",\n".join(json.dumps(name) + ": {" + ",\n".join(
            json.dumps(s) + ": {\n" + ",\n".join(json.dumps(k) + ":" + json.dumps(v, separators=(",", ":"))
                                                for k, v in recs.items()) + "}"
            for s, recs in stored(name, trace(name)).items()) + "}" for name in CORPUS) + "}\n")
    print(GOLDEN, os.path.getsize(GOLDEN), "bytes")
