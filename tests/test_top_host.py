"""The host side of the exact top-k (no GPU): the binding's constants against the header,
HistogramEngine.top's argument mapping against a stub library, TopStatsHandler's parameter
parsing and JSON layout against a stub engine, and the null-context guard of the two C
entry points.
"""
import ctypes
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from linkerd_amd import _native as N
from linkerd_amd.telemetry import MetricsTree, MetricsTreeStatsReceiver
from linkerd_amd.top import BadParameter, TopStatsHandler, parse_params, write_top_json

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(N.HEADER_PATH).read()


def test_constants_match_the_header():
    h = _header()
    assert int(re.search(r"#define L5DH_TOP_LIMIT (\d+)", h).group(1)) == N.TOP_LIMIT == 1024
    enum = dict((k, int(v)) for k, v in re.findall(r"(L5DH_(?:BY|TOP)_[A-Z0-9]+) = (\d+)", h))
    for i, f in enumerate(N.SUMMARY_FIELDS):
        assert enum[f"L5DH_BY_{f.upper()}"] == getattr(N, f"BY_{f.upper()}") == i
    assert enum["L5DH_BY_QUANTILE"] == N.BY_QUANTILE == len(N.SUMMARY_FIELDS) == 11
    assert (enum["L5DH_TOP_LARGEST"], enum["L5DH_TOP_SMALLEST"]) == (N.TOP_LARGEST, N.TOP_SMALLEST) == (0, 1)
    # no new enum name falls into the families tests/test_abi.py collects
    assert not [k for k in enum if k.startswith(("L5DH_K_", "L5DH_PARAM_"))]
    hpp = open(os.path.join(REPO, "linkerd_amd", "csrc", "l5dh_top.hpp")).read()
    assert int(re.search(r"TOP_CHUNK = (\d+);", hpp).group(1)) == N.TOP_CHUNK
    assert int(re.search(r"TOP_LIMIT = (\d+);", hpp).group(1)) == N.TOP_LIMIT
    assert re.search(r"TOP_MAX_ROWS = \(size_t\)1 << (\d+);", hpp).group(1) == "24" and N.TOP_MAX_ROWS == 1 << 24
    assert {"l5dh_top", "l5dh_top_summaries"} <= set(N.SIGNATURES) and N.SIGNATURES["l5dh_top"][1][4] is ctypes.c_double


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(N.LIB_PATH):
        if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
            pytest.skip("libl5dhist.so not built and no hipcc to build it")
        subprocess.run(["make", "-s", "-C", os.path.join(REPO, "linkerd_amd", "csrc")], check=True)
    return N.load()


def test_null_context_is_einval_without_device(lib):
    ids, n = (ctypes.c_uint32 * 4)(), ctypes.c_uint32(7)
    assert lib.l5dh_top(None, 0, 4, N.BY_P99, 0.5, 0, 1, None, 0, 4, ids, None, None, ctypes.byref(n), None, 1) == -22
    vals = np.zeros(4, N.SUMMARY_DTYPE)
    assert lib.l5dh_top_summaries(None, vals.ctypes.data, 4, N.BY_P99, 0, 1, None, 0, 4, ids, None,
                                  ctypes.byref(n)) == -22
    assert n.value == 7 and list(ids) == [0, 0, 0, 0]


# ---- HistogramEngine.top's argument mapping ---------------------------------------------------
class StubLib:
    """Records the two calls and answers with fixed winners."""

    def __init__(self, n=3):
        self.calls, self.n = [], n

    def _answer(self, k, ids_p, top_p, q_p, n_p):
        m = min(self.n, k)
        ctypes.cast(n_p, ctypes.POINTER(ctypes.c_uint32))[0] = m
        for j in range(m):
            ctypes.cast(ids_p, ctypes.POINTER(ctypes.c_uint32))[j] = 10 + j
            if top_p:
                ctypes.cast(top_p, ctypes.POINTER(ctypes.c_int64))[j * 11] = 100 + j
            if q_p:
                ctypes.cast(q_p, ctypes.POINTER(ctypes.c_int64))[j] = 1000 + j
        return 0

    def l5dh_top(self, ctx, first, count, by, q, order, min_count, group, g, k, ids, top, qo, n_out, series, reset):
        self.calls.append(("top", first, count, by, q, order, min_count, bool(group), g, k, bool(qo), bool(series), reset))
        return self._answer(k, ids, top, qo, n_out)

    def l5dh_top_summaries(self, ctx, values, n, by, order, min_count, group, g, k, ids, top, n_out):
        self.calls.append(("ext", n, by, order, min_count, bool(group), g, k))
        return self._answer(k, ids, top, None, n_out)

    def l5dh_last_error(self, ctx):
        return b"stub"


def stub_engine(S=100, n=3):
    from linkerd_amd.engine import HistogramEngine
    e = HistogramEngine.__new__(HistogramEngine)
    e._lib, e._ctx, e.max_series, e.device = StubLib(n), None, S, 0
    e._stream, e._events = None, []
    return e


def test_top_maps_field_names_and_quantiles():
    e = stub_engine()
    for i, f in enumerate(N.SUMMARY_FIELDS):
        ids, summ = e.top(5, f)
        assert e._lib.calls[-1] == ("top", 0, 100, i, 0.0, N.TOP_LARGEST, 1, False, 0, 5, False, False, 0)
        assert ids.dtype == np.uint32 and ids.tolist() == [10, 11, 12] and summ["count"].tolist() == [100, 101, 102]
    ids, summ, qv = e.top(2, 0.995, order="smallest", min_count=0, first=10, count=20, reset=True)
    assert e._lib.calls[-1] == ("top", 10, 20, N.BY_QUANTILE, 0.995, N.TOP_SMALLEST, 0, False, 0, 2, True, False, 1)
    assert ids.tolist() == [10, 11] and qv.tolist() == [1000, 1001] and summ.dtype == N.SUMMARY_DTYPE
    ids, summ, series = e.top(5, "p99", group=np.full(100, -1, np.int64), g=4, with_series=True)
    assert e._lib.calls[-1] == ("top", 0, 100, N.BY_P99, 0.0, 0, 1, True, 4, 5, False, True, 0)
    assert series.shape == (100,) and series.dtype == N.SUMMARY_DTYPE
    assert e.top(5, np.float64(0.25))[2].tolist() == [1000, 1001, 1002]   # a numpy float is a quantile too
    assert e.top(1024)[0].size == 3 and e._lib.calls[-1][3] == N.BY_P99   # the default: by p99


def test_top_rejects_bad_arguments_before_the_library():
    e = stub_engine()
    bad = [dict(by="p98"), dict(by="P99"), dict(by=None), dict(by=b"p99"), dict(order="biggest"), dict(order=0),
           dict(k=0), dict(k=N.TOP_LIMIT + 1), dict(first=50, count=51), dict(group=np.zeros(99, np.uint32)),
           dict(group=np.zeros(100, np.float32)), dict(group=np.full(100, -2, np.int64))]
    for kw in bad:
        with pytest.raises(ValueError):
            e.top(**{"k": 5, **kw})
    assert e._lib.calls == []


def test_top_summaries_mapping():
    e = stub_engine()
    v = np.zeros(40, N.SUMMARY_DTYPE)
    ids, summ = e.top_summaries(v, 2, "avg", order="smallest", min_count=3, group=np.zeros(40, np.uint32), g=0)
    assert e._lib.calls[-1] == ("ext", 40, N.BY_AVG, N.TOP_SMALLEST, 3, True, 0, 2)
    assert ids.tolist() == [10, 11]
    e.top_summaries(v.view(np.int64).reshape(-1), 7, "sum")              # int64 [n * 11] is the same rows
    assert e._lib.calls[-1] == ("ext", 40, N.BY_SUM, 0, 1, False, 0, 7)
    for kw in (dict(by=0.5), dict(by="p98"), dict(k=0)):
        with pytest.raises(ValueError):
            e.top_summaries(v, **{"k": 5, "by": "p99", **kw})
    with pytest.raises(ValueError):
        e.top_summaries(np.zeros(12, np.int64), 5, "p99")                 # not whole summaries
    with pytest.raises(ValueError):
        e.top_into(5, "p99", np.zeros(5, np.uint32), np.zeros(1, np.uint32), values=v, reset=True)


# ---- TopStatsHandler -------------------------------------------------------------------------------
def test_parse_params():
    assert parse_params("/admin/metrics/top.json") == ("p99", 20, "largest", 1, None)
    assert parse_params("/x?by=avg&k=1024&order=smallest&min_count=0&q=rt/http") == ("avg", 1024, "smallest", 0, "rt/http")
    assert parse_params("/x?by=q0.995")[0] == 0.995 and parse_params("/x?by=q1")[0] == 1.0
    assert parse_params("/x?by=q0")[0] == 0.0 and parse_params("/x?by=q1e-3")[0] == 0.001
    for bad in ("by=p98", "by=", "by=q", "by=q1.0001", "by=q-0.1", "by=qnan", "by=qinf", "k=0", "k=1025", "k=-1", "k=x",
                "k=1.5", "order=up", "order=", "min_count=-1", "min_count=x"):
        with pytest.raises(BadParameter):
            parse_params("/x?" + bad)


class StubStatEngine:
    """StatEngine.top's face over fixed rows: ranks nothing, answers what it was built with."""

    def __init__(self, ids, summ, qv=None, capacity=64):
        self.ids, self.summ, self.qv, self.capacity, self.calls = ids, summ, qv, capacity, []

    def top(self, k, by="p99", order="largest", min_count=1, group=None, g=0):
        self.calls.append((k, by, order, min_count, None if group is None else group.copy(), g))
        res = (self.ids[:k], self.summ[:k])
        return res + ((self.qv[:k],) if isinstance(by, float) else ())


def test_handler_layout_and_statuses():
    tree = MetricsTree()
    stats = MetricsTreeStatsReceiver(tree)
    names = [("rt", "http", "client", 'a"b', "latency_ms"), ("rt", "http", "client", "c", "latency_ms"),
             ("rt", "h2", "latency_ms"), ("plain",)]
    for sid, path in enumerate(names):
        stats.stat(*path).series_id = sid   # (no engine attached: the ids are given here)
    summ = np.zeros(3, N.SUMMARY_DTYPE)
    summ[0] = (3, -5, 2147483647, -2 ** 63, 1, 2, 3, 4, 5, 6, float("nan"))
    summ[1] = (1, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7.0)
    summ[2] = (2 ** 40, 0, 9, 2 ** 62, 1, 1, 1, 1, 1, 9, 2.82879384806159e17)
    ids = np.array([2, 0, 1], np.uint32)
    eng = StubStatEngine(ids, summ, np.array([11, 22, 33], np.int64))
    h = TopStatsHandler(tree, eng)
    status, media, body = h.handle("/admin/metrics/top.json?k=3")
    assert (status, media) == (200, "application/json")
    assert body == (
        '[{"name":"rt/h2/latency_ms","count":3,"max":2147483647,"min":-5,"p50":1,"p90":2,"p95":3,"p99":4,"p9990":5,'
        '"p9999":6,"sum":-9223372036854775808,"avg":"NaN"},'
        '{"name":"rt/http/client/a\\"b/latency_ms","count":1,"max":7,"min":7,"p50":7,"p90":7,"p95":7,"p99":7,"p9990":7,'
        '"p9999":7,"sum":7,"avg":7.0},'
        '{"name":"rt/http/client/c/latency_ms","count":1099511627776,"max":9,"min":0,"p50":1,"p90":1,"p95":1,"p99":1,'
        '"p9990":1,"p9999":9,"sum":4611686018427387904,"avg":2.82879384806159008E17}]')
    assert [d["name"] for d in json.loads(body)] == ["rt/h2/latency_ms", 'rt/http/client/a"b/latency_ms',
                                                     "rt/http/client/c/latency_ms"]
    assert eng.calls[-1][:4] == (3, "p99", "largest", 1) and eng.calls[-1][4] is None
    # by a quantile: its value closes each object; k cuts the list
    status, _, body = h.handle("/admin/metrics/top.json?by=q0.995&k=2&order=smallest&min_count=5")
    got = json.loads(body)
    assert status == 200 and [d["quantile"] for d in got] == [11, 22] and list(got[0])[-2:] == ["avg", "quantile"]
    assert eng.calls[-1][:4] == (2, 0.995, "smallest", 5)
    # a subtree: the member map holds 0 for the Stats below it and NO_GROUP elsewhere
    status, _, _ = h.handle("/admin/metrics/top.json?q=rt/http")
    group = eng.calls[-1][4]
    assert status == 200 and group.dtype == np.uint32 and group.shape == (64,) and eng.calls[-1][5] == 0
    assert group[:4].tolist() == [0, 0, N.NO_GROUP, N.NO_GROUP] and (group[4:] == N.NO_GROUP).all()
    # min_count = 0 keeps rows that no Stat owns out
    h.handle("/admin/metrics/top.json?min_count=0")
    assert eng.calls[-1][4][:5].tolist() == [0, 0, 0, 0, N.NO_GROUP]
    n = len(eng.calls)
    assert h.handle("/admin/metrics/top.json?q=rt/nope") == (404, "application/json",
                                                             '{"error": "No such subtree: rt/nope"}')
    status, media, body = h.handle("/admin/metrics/top.json?by=p98")
    assert (status, media) == (400, "application/json") and set(json.loads(body)) == {"error"}
    assert h.handle("/admin/metrics/top.json?k=2000")[0] == 400 and len(eng.calls) == n   # the engine was not asked
    assert write_top_json([]) == "[]"
