"""The host side of the JSON and scalar blocks of the device renderer, on CPU:
l5dh_format_float (the function the kernels compile too) against javafmt.float_to_string,
the same header as a stand-alone program under ASan + UBSan, and the name tables of
admin_metrics.flat_name_table / prometheus.scalar_name_table, pinned by composing
write_flat_json's document and write_scalar_metrics' lines from a table in pure Python.
"""
import ctypes
import errno
import json
import math
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from linkerd_amd import _native as N
from linkerd_amd.admin_metrics import STAT_FIELDS, flat_name_table, scalar_values, write_flat_json
from linkerd_amd.javafmt import double_to_string, float_to_string
from linkerd_amd.prometheus import NO_INDEX, NameTable, scalar_name_table, write_scalar_metrics
from linkerd_amd.telemetry import HistogramSummary, MetricsTreeStatsReceiver

from .test_fmt_host import ONE_TWO, exporters_tree, labels, lib, row_texts  # noqa: F401  (lib: the fixture)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")

FLT_MAX = float(np.finfo(np.float32).max)
LEAST = float(np.float32(2.0 ** -149))


def f32(x) -> float:
    return float(np.float32(x))


def bits_of(x: float) -> int:
    return struct.unpack("<I", struct.pack("<f", x))[0]


def of_bits(b: int) -> float:
    return struct.unpack("<f", struct.pack("<I", b))[0]


def in_min_domain(x: float) -> bool:
    """What l5dh_format_float takes at the least: +-0.0, NaN, +-Infinity, finite 2^-64 <= |x| < 2^64."""
    return x != x or math.isinf(x) or x == 0.0 or 2.0 ** -64 <= abs(x) < 2.0 ** 64


def fmt_float(lib, x):
    """(status, text) of l5dh_format_float; the buffer is exactly L5DH_FLOAT_CHARS."""
    buf, n = ctypes.create_string_buffer(N.FLOAT_CHARS), ctypes.c_size_t(99)
    rc = lib.l5dh_format_float(ctypes.c_float(x), buf, ctypes.byref(n))
    return rc, buf.raw[:n.value].decode()


def check_floats(lib, xs):
    """Inside the minimum domain: never refused, equal to javafmt.  Outside: equal, or
    -ERANGE with *len == 0.  Returns how many were refused."""
    refused = 0
    for x in xs:
        rc, text = fmt_float(lib, x)
        if rc == 0:
            assert text == float_to_string(x), repr(x)
        else:
            assert not in_min_domain(x), f"{x!r} is inside the domain and was refused ({rc})"
            assert rc == -errno.ERANGE and text == "", repr(x)
            refused += 1
    return refused


def edge_floats():
    below = float(np.nextafter(np.float32(2.0 ** -64), np.float32(0)))
    pos = [0.0, float("nan"), float("inf"), 1e7, 9999999.0, f32(0.001), f32(9.999e-4), 2.0 ** 24 - 1, 2.0 ** 24,
           2.0 ** 24 + 2, f32(2.0 ** 24 + 1), f32(1.48832833e12), f32(4008938.8), 2.0 ** -64, below, 2.0 ** 64, FLT_MAX,
           LEAST, float(np.finfo(np.float32).tiny), f32(1e-45), f32(3.4e38), f32(1e10), f32(0.1), f32(1 / 3)]
    pos += [2.0 ** k for k in range(-64, 64)]  # every power of two inside the minimum domain
    pos += [2.0 ** k for k in range(-149, -64)] + [2.0 ** k for k in range(64, 128)]  # and outside it
    return pos + [-x for x in pos if x == x]


def test_format_float_fixture_gauges(lib):
    texts = json.load(open(os.path.join(GOLDEN, "p5_number_texts.json")))["texts"]
    gauges = [t["text"].replace("E+", "E") for t in texts if t["key"] == "gauge"]
    assert len(gauges) > 200
    for g in gauges:
        assert fmt_float(lib, float(g)) == (0, g)


def test_format_float_random_bit_patterns(lib):
    """50 000 random floats of the minimum domain: none refused, each equals javafmt."""
    rng = np.random.default_rng(24)
    # sign, a biased exponent of 2^-64 .. 2^63, any fraction
    b = (rng.integers(0, 2, 50_000) << 31) | (rng.integers(127 - 64, 127 + 64, 50_000) << 23) | rng.integers(0, 1 << 23, 50_000)
    xs = [of_bits(int(v)) for v in b]
    assert all(in_min_domain(x) and x == x and x != 0.0 for x in xs)
    assert check_floats(lib, xs) == 0


def test_format_float_edges(lib):
    xs = edge_floats()
    check_floats(lib, xs)
    assert fmt_float(lib, 0.0) == (0, "0.0") and fmt_float(lib, -0.0) == (0, "-0.0")
    assert fmt_float(lib, float("nan")) == (0, "NaN")
    assert fmt_float(lib, float("inf")) == (0, "Infinity") and fmt_float(lib, -float("inf")) == (0, "-Infinity")
    assert fmt_float(lib, 1e7) == (0, "1.0E7") and fmt_float(lib, 9999999.0) == (0, "9999999.0")
    assert fmt_float(lib, f32(0.001)) == (0, "0.001") and fmt_float(lib, f32(9.999e-4)) == (0, "9.999E-4")
    assert fmt_float(lib, 2.0 ** 24 - 1) == (0, "1.6777215E7") and fmt_float(lib, 2.0 ** 24 + 2) == (0, "1.6777218E7")
    assert fmt_float(lib, f32(1.48832833e12)) == (0, "1.48832833E12")  # digits the shortest form drops
    assert fmt_float(lib, f32(4008938.8)) == (0, "4008938.8")
    assert fmt_float(lib, 2.0 ** -64) == (0, "5.421011E-20") and fmt_float(lib, 2.0 ** 63) == (0, "9.223372E18")
    # the header derives that the formatter's integer covers every float: none is refused
    assert fmt_float(lib, FLT_MAX) == (0, "3.4028235E38") and fmt_float(lib, LEAST) == (0, "1.4E-45")
    assert fmt_float(lib, float(np.finfo(np.float32).tiny)) == (0, "1.17549435E-38")
    assert max(len(float_to_string(x)) for x in xs) < N.FLOAT_CHARS


def test_format_float_whole_range_sample(lib):
    """Outside the minimum domain a value equals javafmt or is refused -- never another text."""
    rng = np.random.default_rng(25)
    xs = [of_bits(int(v)) for v in rng.integers(0, 1 << 32, 20_000)]
    xs += [of_bits(m) for m in range(1, 300)] + [of_bits((1 << 23) - m) for m in range(1, 300)]  # subnormals
    check_floats(lib, xs)


def test_format_float_rejects_null_arguments(lib):
    n = ctypes.c_size_t(0)
    assert lib.l5dh_format_float(ctypes.c_float(1.0), None, ctypes.byref(n)) == -errno.EINVAL
    assert lib.l5dh_format_float(ctypes.c_float(1.0), ctypes.create_string_buffer(N.FLOAT_CHARS), None) == -errno.EINVAL


def test_insignificant_digits_formula():
    """l5dh_fmt.hpp takes INSIGNIFICANT_DIGITS[p2] as (p2 * 1233) >> 12 on the exact-long path."""
    from linkerd_amd.javafmt import INSIGNIFICANT_DIGITS
    assert [(p2 * 1233) >> 12 for p2 in range(63)] == INSIGNIFICANT_DIGITS[:63]


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ absent")
def test_fmt_header_asan_ubsan(tmp_path):
    """l5dh_fmt.hpp as plain C++ in a stand-alone program (tests/c/fmt_float_check.cpp) under
    ASan + UBSan on the CPU: clean, and the edge list's texts equal javafmt."""
    exe = tmp_path / "fmt_float_check"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-o", str(exe), os.path.join(REPO, "tests", "c", "fmt_float_check.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    floats = edge_floats()
    doubles = [float(x) for x in floats if in_min_domain(x)] + [2.82879384806159e17, 1e23, 5e-324]
    lines = ["f %08x" % bits_of(x) for x in floats]
    lines += ["d %016x" % struct.unpack("<Q", struct.pack("<d", x))[0] for x in doubles]
    r = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0 and "runtime error" not in r.stderr and r.stderr == "", r.stderr[-4000:]
    got = r.stdout.split("\n")[:-1]
    assert len(got) == len(lines)
    for x, text in zip(floats, got):
        assert text == float_to_string(x) or (text == "ERANGE" and not in_min_domain(x)), repr(x)
    for x, text in zip(doubles, got[len(floats):]):
        assert text == (double_to_string(x) if 2.0 ** -64 <= abs(x) < 2.0 ** 64 or x == 0 or x != x or math.isinf(x)
                        else "ERANGE"), repr(x)


# ---- name tables ---------------------------------------------------------------------
WEIRD = 'we"ird\\na\nme\x01/é√'  # a quote, a backslash, a newline, a control character, non-ASCII
EMPTY = HistogramSummary(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0.0)


def json_number(text: str) -> str:
    return '"' + text + '"' if text in ("NaN", "Infinity", "-Infinity") else text


def json_entries(table, j, m):
    """What the device composes for row j: `"key sfx":number,` per entry."""
    key, _ = row_texts(table, j)
    kind = int(table.kinds[j])
    if kind == N.KIND_COUNTER:
        return [f'"{key}":{int(m.get())},']
    if kind == N.KIND_GAUGE:
        return [f'"{key}":{json_number(float_to_string(m.get()))},']
    s = m.snapshotted_summary
    out = [f'"{key}.count":{s.count},']
    if s.count > 0:
        out += [f'"{key}.{f}":{getattr(s, f)},' for f in STAT_FIELDS]
        out.append(f'"{key}.avg":{json_number(double_to_string(s.avg))},')
    return out


def json_document(table):
    text = "".join(e for j, m in enumerate(table.metrics)
                   if table.kinds[j] != N.KIND_STAT or m.snapshotted_summary is not None
                   for e in json_entries(table, j, m))
    return "{" + text[:-1] + "}"


def scrape_tree():
    """test_fmt_host's exporters tree plus counters and gauges (one NaN, one infinite), a
    Stat with count == 0, the never-snapshotted Stat it already has, and a weird name."""
    tree, made = exporters_tree()
    stats = MetricsTreeStatsReceiver(tree)
    stats.scope("rt", "incoming").counter("failures").incr(2 ** 40)
    stats.scope(WEIRD).counter("requests").incr(7)
    values = {"heap": 1.48832833e12, "nan": float("nan"), "inf": -float("inf"), "zero": -0.0, "small": 9.999e-4}
    for name, v in values.items():
        stats.scope("jvm", WEIRD).add_gauge(name, f=lambda v=v: v)
    stats.scope("foo").stat("empty")._set_snapshot(EMPTY)
    stats.scope(WEIRD).stat("lat")._set_snapshot(ONE_TWO)
    return tree


def test_flat_name_table_composes_write_flat_json():
    tree = scrape_tree()
    table = flat_name_table(tree)
    kinds = table.kinds.tolist()
    assert table.kinds.dtype == np.uint8 and len(kinds) == table.n == len(table.metrics)
    assert kinds.count(N.KIND_COUNTER) == 3 and kinds.count(N.KIND_GAUGE) == 5 and kinds.count(N.KIND_STAT) == 12
    for kind in (N.KIND_COUNTER, N.KIND_GAUGE):  # a scalar's index is its ordinal among its kind
        assert table.index[table.kinds == kind].tolist() == list(range(kinds.count(kind)))
    assert table.index[table.kinds == N.KIND_STAT].tolist() == [NO_INDEX] * 12  # no engine: no series ids
    assert int(table.lab_off[-1]) == 0 and table.key_off[-1] == table.key_bytes.size
    want = write_flat_json(tree)
    assert json_document(table) == want
    assert '"we\\"ird\\\\na\\nme\\u0001/é√/requests":7' in want and '"foo/empty.count":0' in want
    assert '"foo/empty.max"' not in want
    assert '/nan":"NaN"' in want and '/inf":"-Infinity"' in want and '/zero":-0.0' in want
    assert "never_snapshotted" not in want and '"rt/incoming/failures":1099511627776' in want
    counters, gauges = scalar_values(table)
    assert counters.dtype == np.int64 and gauges.dtype == np.float32
    assert sorted(counters.tolist()) == [3, 7, 2 ** 40] and gauges.size == 5
    for j, m in enumerate(table.metrics):
        if kinds[j] == N.KIND_COUNTER:
            assert counters[table.index[j]] == m.get()
        elif kinds[j] == N.KIND_GAUGE:
            assert float_to_string(float(gauges[table.index[j]])) == float_to_string(m.get())


def test_scalar_name_table_composes_write_scalar_metrics():
    tree = scrape_tree()
    table = scalar_name_table(tree)
    counters, gauges = scalar_values(table)
    assert table.n == 8 and counters.size == 3 and gauges.size == 5
    lines = []
    for j in range(table.n):
        key, inner = row_texts(table, j)
        i = int(table.index[j])
        value = str(int(counters[i])) if table.kinds[j] == N.KIND_COUNTER else float_to_string(float(gauges[i]))
        lines.append(f"{key}{labels(inner)} {value}\n")
    want = []
    write_scalar_metrics(tree, want)
    assert lines == want and len(want) == 8
    text = "".join(want)
    assert 'rt:failures{rt="incoming"} 1099511627776\n' in text and ":nan NaN\n" in text and ":zero -0.0\n" in text


def test_take_and_to_device_keep_kinds(monkeypatch):
    table = flat_name_table(scrape_tree())
    part = table.take([5, 0, 5])
    assert part.kinds.tolist() == [table.kinds[5], table.kinds[0], table.kinds[5]] and part.kinds.dtype == np.uint8
    assert row_texts(part, 2) == row_texts(table, 5) and part.metrics[1] is table.metrics[0]
    assert NameTable.build(["a"], [""]).kinds is None and NameTable.build(["a"], [""]).take([0]).kinds is None
    # to_device sends every array through torch: with torch's calls replaced, kinds goes the same way
    import torch

    class Dev:
        def __init__(self, a):
            self.a = a

        def to(self, dev):
            return ("on", str(dev), self.a)
    monkeypatch.setattr(torch, "from_numpy", lambda a: Dev(a))
    dev = table.to_device(0)
    assert dev.kinds[:2] == ("on", "cuda:0") and np.array_equal(dev.kinds[2], table.kinds)
    assert dev.index[0] == "on" and dev.metrics is table.metrics
