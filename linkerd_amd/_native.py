"""ctypes binding of the C-ABI in include/l5dhist.h (linkerd_amd/lib/libl5dhist.so).

This is the same boundary a JVM would bind through JNI.  There
is no fallback: if the HIP library is missing, importing the engine raises.
"""
from __future__ import annotations

import ctypes
import errno
import os
import re
import threading

import numpy as np

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
REPO_DIR = os.path.dirname(PKG_DIR)
# L5DH_LIB selects another build of the same library (A/B timing of kernel variants: tools/ab.sh)
LIB_PATH = os.environ.get("L5DH_LIB") or os.path.join(PKG_DIR, "lib", "libl5dhist.so")
SYNTH_PATH = os.path.join(PKG_DIR, "lib", "libl5dsynth.so")
HEADER_PATH = os.path.join(REPO_DIR, "include", "l5dhist.h")

NLIMITS = 1797
NBUCKETS = 1798
SUMMARY_FIELDS = ("count", "min", "max", "sum", "p50", "p90", "p95", "p99", "p9990", "p9999", "avg")
SUMMARY_DTYPE = np.dtype([(f, "<i8") for f in SUMMARY_FIELDS[:-1]] + [("avg", "<f8")])
BUCKET_COUNT_DTYPE = np.dtype([("lower", "<i4"), ("upper", "<i4"), ("count", "<i4")])
BUCKET_ENTRY_DTYPE = np.dtype([("bucket", "<u4"), ("count", "<u4")])  # l5dh_bucket_entry

PARAM_TIMING = 1
PARAM_COLD_LIMIT = 2
PARAM_HOT_CHUNK = 3
PARAM_MAX_SEGMENTS = 4
PARAM_DIRECT_MAX = 6
PARAM_DIRECT_DIV = 7
PARAM_STAGE_SAMPLES = 9
PARAM_MAX_SLABS = 10
PARAM_MERGE_RCCL_1RANK = 11
PARAM_VARIANT = 12
PARAM_REGION_PCT = 13
PARAM_ROLLUP_ITEM = 14

NO_GROUP = 0xFFFFFFFF  # L5DH_NO_GROUP
MAX_SERIES = 1 << 20  # L5DH_MAX_SERIES
LE_MAX = 64  # L5DH_LE_MAX
Q_MAX = 64  # L5DH_Q_MAX
WINDOW_MAX = 64  # L5DH_WINDOW_MAX: slots of a sliding window
MAX_COUNTERS = 1 << 24  # L5DH_MAX_COUNTERS: counters of a context's counter space
VARIANT_COUNTERS_PLAIN = 8  # L5DH_PARAM_VARIANT bit 3: counters_add without the LDS claim table
DOUBLE_CHARS = 26  # L5DH_DOUBLE_CHARS
FLOAT_CHARS = 16  # L5DH_FLOAT_CHARS
KIND_COUNTER, KIND_GAUGE, KIND_STAT = 0, 1, 2  # L5DH_KIND_*: a row's kind in render_json / render_scalars
LONG_CHARS = 20  # L5DH_LONG_CHARS

# top-k selection (l5dh_top, l5dh_top_summaries; the kernels' constants: csrc/l5dh_top.hpp)
TOP_LIMIT = 1024  # L5DH_TOP_LIMIT: k per call
TOP_CHUNK = 4096  # rows one workgroup of the tournament sorts
TOP_MAX_ROWS = 1 << 24  # rows of one external selection
(BY_COUNT, BY_MIN, BY_MAX, BY_SUM, BY_P50, BY_P90, BY_P95, BY_P99, BY_P9990, BY_P9999, BY_AVG,
 BY_QUANTILE) = range(12)  # L5DH_BY_*: the field's index in SUMMARY_FIELDS; BY_QUANTILE: percentile(q), live only
TOP_LARGEST, TOP_SMALLEST = 0, 1  # L5DH_TOP_*


class Names(ctypes.Structure):
    """l5dh_names: the five arrays of a name table (host or device addresses; 0: NULL)."""
    _fields_ = [("index", ctypes.c_void_p), ("key_off", ctypes.c_void_p), ("key_bytes", ctypes.c_void_p),
                ("lab_off", ctypes.c_void_p), ("lab_bytes", ctypes.c_void_p)]


class InfluxNames(ctypes.Structure):
    """l5dh_influx_names: the ten arrays of an InfluxDB table (render_influx.InfluxTable)."""
    _fields_ = [(f, ctypes.c_void_p) for f in ("line", "kinds", "field", "index", "key_off", "key_bytes", "head_off",
                                               "head_bytes", "tail_off", "tail_bytes")]


MERGE_REDUCE_SCATTER = 0
MERGE_ALL_REDUCE = 1
UNIQUE_ID_BYTES = 128
OWN_STREAM = ctypes.c_void_p(-1 & (2 ** 64 - 1)).value  # L5DH_OWN_STREAM

K_COUNT, K_SCAN, K_BIN, K_ACCUM, K_HOT, K_COPY, K_BIN2, K_MERGE, K_WINDOW, K_COUNTERS = range(10)
KERNEL_NAMES = ("count", "scan", "bin1", "accum", "hot", "copy", "bin2", "merge", "window", "counters")


class NativeLibraryMissing(ImportError):
    pass


class L5dhError(RuntimeError):
    def __init__(self, code: int, where: str, detail: str = ""):
        self.code = code
        name = errno.errorcode.get(-code, str(code)) if code < 0 else str(code)
        super().__init__(f"{where} failed: {name} ({code}) {detail}".rstrip())


_lock = threading.Lock()
_lib = None

_c = ctypes
_vp = _c.c_void_p
SIGNATURES = {
    "l5dh_abi_version": (_c.c_int, []),
    "l5dh_open": (_c.c_int, [_c.POINTER(_vp), _c.c_uint32, _c.c_uint32]),
    "l5dh_close": (_c.c_int, [_vp]),
    "l5dh_limits": (_c.POINTER(_c.c_int32), [_c.POINTER(_c.c_size_t)]),
    "l5dh_ingest": (_c.c_int, [_vp, _vp, _vp, _c.c_size_t]),
    "l5dh_ingest_async": (_c.c_int, [_vp, _vp, _vp, _c.c_size_t, _c.POINTER(_c.c_uint64)]),
    "l5dh_ingest_wait": (_c.c_int, [_vp, _c.c_uint64]),
    "l5dh_snapshot": (_c.c_int, [_vp, _c.c_uint32, _c.c_uint32, _vp, _vp, _c.c_int]),
    "l5dh_peek": (_c.c_int, [_vp, _c.c_uint32, _vp, _c.c_size_t, _c.POINTER(_c.c_size_t)]),
    "l5dh_export_state": (_c.c_int, [_vp, _c.c_uint32, _c.c_uint32, _vp, _vp, _c.c_int]),
    "l5dh_summarize_dense": (_c.c_int, [_vp, _vp, _vp, _c.c_size_t, _vp]),
    "l5dh_rollup": (_c.c_int, [_vp, _c.c_uint32, _c.c_uint32, _vp, _c.c_uint32, _vp, _vp, _vp, _vp, _c.c_int]),
    "l5dh_rollup_dense": (_c.c_int, [_vp, _vp, _vp, _c.c_size_t, _vp, _c.c_uint32, _vp, _vp, _vp]),
    "l5dh_le_cuts": (_c.c_int, [_vp, _c.c_size_t, _vp, _vp]),
    "l5dh_le": (_c.c_int, [_vp, _c.c_uint32, _c.c_uint32, _vp, _c.c_uint32, _vp, _vp, _c.c_int, _vp, _c.c_int]),
    "l5dh_le_dense": (_c.c_int, [_vp, _vp, _vp, _c.c_size_t, _vp, _c.c_uint32, _vp, _vp, _c.c_int]),
    "l5dh_quantiles": (_c.c_int, [_vp, _c.c_uint32, _c.c_uint32, _vp, _c.c_uint32, _vp, _vp, _c.c_int]),
    "l5dh_quantiles_dense": (_c.c_int, [_vp, _vp, _c.c_size_t, _vp, _c.c_uint32, _vp]),
    "l5dh_top": (_c.c_int, [_vp, _c.c_uint32, _c.c_uint32, _c.c_int, _c.c_double, _c.c_int, _c.c_int64, _vp, _c.c_uint32,
                            _c.c_uint32, _vp, _vp, _vp, _vp, _vp, _c.c_int]),
    "l5dh_top_summaries": (_c.c_int, [_vp, _vp, _c.c_size_t, _c.c_int, _c.c_int, _c.c_int64, _vp, _c.c_uint32,
                                      _c.c_uint32, _vp, _vp, _vp]),
    "l5dh_import_state": (_c.c_int, [_vp, _c.c_uint32, _c.c_uint32, _vp, _vp]),
    "l5dh_export_sparse": (_c.c_int, [_vp, _c.c_uint32, _c.c_uint32, _vp, _vp, _c.c_size_t, _c.POINTER(_c.c_size_t),
                                      _vp, _c.c_int]),
    "l5dh_import_sparse": (_c.c_int, [_vp, _vp, _c.c_uint32, _c.c_size_t, _vp, _vp, _vp]),
    "l5dh_window_open": (_c.c_int, [_vp, _c.c_uint32]),
    "l5dh_window_close": (_c.c_int, [_vp]),
    "l5dh_window_push": (_c.c_int, [_vp, _c.c_uint32, _vp]),
    "l5dh_window_query": (_c.c_int, [_vp, _c.c_uint32, _c.c_uint32, _c.c_uint32, _c.c_int, _vp, _vp, _vp]),
    "l5dh_window_forget": (_c.c_int, [_vp, _c.c_uint32, _c.c_uint32]),
    "l5dh_window_move": (_c.c_int, [_vp, _vp]),
    "l5dh_window_info": (_c.c_int, [_vp, _c.POINTER(_c.c_uint32), _c.POINTER(_c.c_uint32), _c.POINTER(_c.c_uint64),
                                    _c.POINTER(_c.c_uint64), _c.POINTER(_c.c_uint64)]),
    "l5dh_counters_open": (_c.c_int, [_vp, _c.c_uint32]),
    "l5dh_counters_close": (_c.c_int, [_vp]),
    "l5dh_counters_resize": (_c.c_int, [_vp, _c.c_uint32]),
    "l5dh_counters_add": (_c.c_int, [_vp, _vp, _vp, _c.c_size_t]),
    "l5dh_counters_read": (_c.c_int, [_vp, _c.c_uint32, _c.c_uint32, _vp]),
    "l5dh_counters_write": (_c.c_int, [_vp, _c.c_uint32, _c.c_uint32, _vp]),
    "l5dh_counters_rollup": (_c.c_int, [_vp, _c.c_uint32, _c.c_uint32, _vp, _c.c_uint32, _vp]),
    "l5dh_counters_values": (_c.c_int, [_vp, _c.POINTER(_vp), _c.POINTER(_c.c_uint32)]),
    "l5dh_counters_move": (_c.c_int, [_vp, _vp]),
    "l5dh_counters_info": (_c.c_int, [_vp, _c.POINTER(_c.c_uint32), _c.POINTER(_c.c_uint64), _c.POINTER(_c.c_uint64),
                                      _c.POINTER(_c.c_uint64), _c.POINTER(_c.c_uint64)]),
    "l5dh_format_double": (_c.c_int, [_c.c_double, _vp, _c.POINTER(_c.c_size_t)]),
    "l5dh_format_float": (_c.c_int, [_c.c_float, _vp, _c.POINTER(_c.c_size_t)]),
    "l5dh_format_long": (_c.c_int, [_c.c_int64, _vp, _c.POINTER(_c.c_size_t)]),
    "l5dh_format_ulong": (_c.c_int, [_c.c_uint64, _vp, _c.POINTER(_c.c_size_t)]),
    "l5dh_render_summaries": (_c.c_int, [_vp, _vp, _c.c_size_t, _vp, _c.c_size_t, _vp, _c.c_size_t,
                                         _c.POINTER(_c.c_size_t)]),
    "l5dh_render_le": (_c.c_int, [_vp, _vp, _c.c_size_t, _vp, _vp, _c.c_size_t, _vp, _c.c_uint32, _vp, _c.c_size_t,
                                  _c.POINTER(_c.c_size_t)]),
    "l5dh_render_quantiles": (_c.c_int, [_vp, _vp, _c.c_size_t, _vp, _c.c_size_t, _vp, _c.c_uint32, _vp, _c.c_size_t,
                                         _c.POINTER(_c.c_size_t)]),
    "l5dh_render_json": (_c.c_int, [_vp, _vp, _vp, _c.c_size_t, _vp, _c.c_size_t, _vp, _c.c_size_t, _vp, _c.c_size_t,
                                    _vp, _c.c_size_t, _c.POINTER(_c.c_size_t)]),
    "l5dh_render_scalars": (_c.c_int, [_vp, _vp, _vp, _c.c_size_t, _vp, _c.c_size_t, _vp, _c.c_size_t, _vp,
                                       _c.c_size_t, _c.POINTER(_c.c_size_t)]),
    "l5dh_render_influx": (_c.c_int, [_vp, _vp, _c.c_size_t, _c.c_size_t, _vp, _c.c_size_t, _vp, _c.c_size_t, _vp,
                                      _c.c_size_t, _vp, _c.c_size_t, _vp, _c.c_size_t, _c.POINTER(_c.c_size_t)]),
    "l5dh_sync": (_c.c_int, [_vp]),
    "l5dh_set_stream": (_c.c_int, [_vp, _vp]),
    "l5dh_wait_event": (_c.c_int, [_vp, _vp]),
    "l5dh_set_param": (_c.c_int, [_vp, _c.c_int, _c.c_int64]),
    "l5dh_kernel_time": (_c.c_int, [_vp, _c.c_int, _c.POINTER(_c.c_double), _c.POINTER(_c.c_int64), _c.c_int]),
    "l5dh_device": (_c.c_int, [_vp, _c.POINTER(_c.c_int)]),
    "l5dh_max_series": (_c.c_uint32, [_vp]),
    "l5dh_pin_alloc": (_c.c_int, [_c.c_size_t, _c.POINTER(_vp)]),
    "l5dh_pin_free": (_c.c_int, [_vp]),
    "l5dh_last_error": (_c.c_char_p, [_vp]),
    "l5dh_comm_unique_id": (_c.c_int, [_vp]),
    "l5dh_comm_init_rank": (_c.c_int, [_vp, _vp, _c.c_int, _c.c_int]),
    "l5dh_comm_init_all": (_c.c_int, [_c.POINTER(_vp), _c.c_int]),
    "l5dh_comm_init_loopback": (_c.c_int, [_c.POINTER(_vp), _c.c_int]),
    "l5dh_comm_destroy": (_c.c_int, [_vp]),
    "l5dh_merge": (_c.c_int, [_vp, _c.c_int, _vp, _vp, _vp, _c.POINTER(_c.c_uint32), _c.POINTER(_c.c_uint32)]),
    "l5dh_tile_totals": (_c.c_int, [_vp, _c.POINTER(_c.c_uint64), _c.c_size_t]),
    "l5dh_merge_bytes": (_c.c_int, [_vp, _c.POINTER(_c.c_uint64), _c.POINTER(_c.c_uint64), _c.POINTER(_c.c_uint64)]),
    "l5dh_partition_redos": (_c.c_int, [_vp, _c.POINTER(_c.c_uint64), _c.POINTER(_c.c_uint64),
                                        _c.POINTER(_c.c_uint64)]),
    "l5dh_merge_all": (_c.c_int, [_c.POINTER(_vp), _c.c_int, _c.c_int, _c.POINTER(_vp), _c.POINTER(_vp),
                                  _c.POINTER(_vp), _c.POINTER(_c.c_uint32), _c.POINTER(_c.c_uint32)]),
}


def engine_source_hash() -> str:
    """sha256 (16 hex) of the engine's kernel and host sources: ties committed
    profiles (PMC traffic) to the code they measured."""
    import hashlib
    h = hashlib.sha256()
    d = os.path.join(PKG_DIR, "csrc")
    for f in sorted(os.listdir(d)):
        if f.endswith((".hip", ".hpp", ".cpp")) and "synth" not in f:
            h.update(f.encode())
            h.update(open(os.path.join(d, f), "rb").read())
    return h.hexdigest()[:16]


def header_symbols(path: str = HEADER_PATH) -> list:
    """Function names declared in include/l5dhist.h."""
    text = open(path).read()
    return sorted(set(re.findall(r"\b(l5dh_[a-z_0-9]+)\s*\(", text)))


def load(path: str = LIB_PATH):
    """Load the HIP engine library; raises NativeLibraryMissing if absent."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        # One HIP runtime per process: torch ships libamdhip64.so with the same
        # soname as /opt/rocm's.  Loading torch first makes our DT_NEEDED resolve
        # to the already-mapped runtime instead of mapping a second one.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        if not os.path.exists(path):
            raise NativeLibraryMissing(
                f"{path} not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                "(or make -C linkerd_amd/csrc); there is no CPU fallback")
        lib = ctypes.CDLL(path)
        for name, (res, args) in SIGNATURES.items():
            if os.environ.get("L5DH_LIB") and not hasattr(lib, name):
                continue  # (an A/B build of an older revision: entry points it predates are absent)
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _lib = lib
        return lib


def limits() -> np.ndarray:
    lib = load()
    n = ctypes.c_size_t(0)
    p = lib.l5dh_limits(ctypes.byref(n))
    if not p or n.value != NLIMITS:
        raise L5dhError(-errno.EIO, "l5dh_limits")
    return np.ctypeslib.as_array(p, shape=(NLIMITS,)).copy()
