"""Host and device arguments give the same bytes.

Every entry point that takes caller arrays uses a device pointer in place and stages a
host pointer through a buffer of the context.  Each call runs twice on identical state
-- numpy arrays, then torch tensors on the GPU -- and both results must equal the CPU
oracle's bytes (integers and the avg's float64 alike: tobytes).  S = 70 is three tiles,
the last ragged; every series and every group holds samples.
"""
import ctypes

import numpy as np
import pytest

from linkerd_amd import _native as N

pytestmark = pytest.mark.gpu

S, G, NSAMP = 70, 5, 20_000


@pytest.fixture(scope="module")
def case(oracle):
    """The batch, the group map and the oracle's results, computed once."""
    rng = np.random.default_rng(7)
    series = rng.integers(0, S, size=NSAMP, dtype=np.uint32)
    vals = np.exp(3.0 + rng.standard_normal(NSAMP)).astype(np.float32)
    vals[:8] = np.array([0, 1, 2, 113, 3030, 1e9, 3e9, -5], dtype=np.float32)  # smoke()'s edge values
    series[:8] = [69, 0, 31, 32, 63, 64, 69, 33]
    ref = oracle.OracleHistograms(S)
    assert ref.ingest(series, vals) == 0
    counts, totals = ref.counts(), ref.totals()
    assert counts.sum(axis=1).all() and counts[:, 0].any() and counts[:, N.NBUCKETS - 1].any()
    group = (np.arange(S) % G).astype(np.uint32)
    gc = np.zeros((G, N.NBUCKETS), np.int64)
    gt = np.zeros(G, np.int64)
    np.add.at(gc, group, counts)
    np.add.at(gt, group, totals)
    gc = gc.astype(np.int32)
    return dict(series=series, vals=vals, counts=counts, totals=totals, group=group,
                summ=oracle.summarize_counts(counts, totals), g_counts=gc, g_totals=gt,
                g_summ=oracle.summarize_counts(gc, gt))


@pytest.fixture(scope="module")
def eng(gpu_available):
    from linkerd_amd.engine import HistogramEngine
    with HistogramEngine(S) as e:
        HistogramEngine.comm_init_loopback([e])  # a 1-rank group, for the merge
        yield e


class Bufs:
    """Output (or input) arrays of one run: numpy, or torch tensors on the GPU."""

    def __init__(self, device):
        self.device = device

    def zeros(self, n, dtype):
        if not self.device:
            return np.zeros(n, dtype)
        import torch
        return torch.zeros(n, dtype=getattr(torch, np.dtype(dtype).name), device="cuda:0")

    def summ(self, rows):  # 11 x 8 bytes per row
        return self.zeros(rows * 11, np.int64)

    def put(self, a):
        if not self.device:
            return a
        import torch
        return torch.from_numpy(a).to("cuda:0")


def raw(x):
    return (x if isinstance(x, np.ndarray) else x.cpu().numpy()).tobytes()


def both(eng, case, call, resets):
    """call(bufs) -> tuple of output arrays; host run, then device run, on the same state."""
    res = []
    for device in (False, True):
        if resets or not device:
            eng.ingest(case["series"], case["vals"])
        res.append([raw(o) for o in call(Bufs(device))])
    if not resets:
        eng.snapshot(reset=True)  # leave the engine empty for the next test
    assert res[0] == res[1], "host and device arguments give different bytes"
    return res[0]


def test_snapshot_into(eng, case):
    def call(b):
        summ, counts = b.summ(S), b.zeros(S * N.NBUCKETS, np.int32)
        eng.snapshot_into(summ, counts, reset=True)
        return summ, counts
    assert both(eng, case, call, True) == [case["summ"].tobytes(), case["counts"].tobytes()]


def test_snapshot_into_misaligned_host_counts(eng, case):
    """A host view 4 bytes into an int64-backed buffer: the staged path of the helper."""
    backing = np.zeros(S * N.NBUCKETS // 2 + 1, np.int64)
    counts = backing.view(np.int32)[1:1 + S * N.NBUCKETS]
    assert counts.ctypes.data % 8 == 4
    summ = np.zeros(S, N.SUMMARY_DTYPE)
    eng.ingest(case["series"], case["vals"])
    eng.snapshot_into(summ, counts, reset=True)
    assert counts.tobytes() == case["counts"].tobytes() and summ.tobytes() == case["summ"].tobytes()
    assert backing.view(np.int32)[0] == 0 and backing.view(np.int32)[-1] == 0


def test_export_state(eng, case):
    def call(b):
        counts, totals = b.zeros(S * N.NBUCKETS, np.int32), b.zeros(S, np.int64)
        eng.export_state(reset=True, counts=counts, totals=totals)
        return counts, totals
    assert both(eng, case, call, True) == [case["counts"].tobytes(), case["totals"].tobytes()]


def test_summarize_dense(eng, case):
    def call(b):
        out = b.summ(S)
        eng.summarize_dense(b.put(case["counts"].reshape(-1)), b.put(case["totals"]), out)
        return (out,)
    assert both(eng, case, call, False) == [case["summ"].tobytes()]


@pytest.mark.parametrize("dense", [False, True])
def test_rollup_into(eng, case, dense):
    def call(b):
        summ, counts, totals = b.summ(G), b.zeros(G * N.NBUCKETS, np.int32), b.zeros(G, np.int64)
        if dense:
            eng.rollup_into(b.put(case["group"]), G, summ, counts, totals,
                            dense=(b.put(case["counts"].reshape(-1)), b.put(case["totals"])))
            return summ, counts, totals
        series = b.summ(S)
        eng.rollup_into(b.put(case["group"]), G, summ, counts, totals, series=series, reset=True)
        return summ, counts, totals, series
    want = [case["g_summ"].tobytes(), case["g_counts"].tobytes(), case["g_totals"].tobytes()]
    assert both(eng, case, call, not dense) == want + ([] if dense else [case["summ"].tobytes()])


@pytest.mark.parametrize("mode", [N.MERGE_REDUCE_SCATTER, N.MERGE_ALL_REDUCE])
def test_merge_one_rank_loopback(eng, case, mode):
    lib = N.load()

    def call(b):
        summ, counts, totals = b.summ(S), b.zeros(S * N.NBUCKETS, np.int32), b.zeros(S, np.int64)
        if b.device:
            eng._order_after_torch()  # (the tensors were zeroed on torch's stream)
        ptr = [(ctypes.c_void_p * 1)(x.ctypes.data if isinstance(x, np.ndarray) else x.data_ptr())
               for x in (summ, counts, totals)]
        first, count = (ctypes.c_uint32 * 1)(), (ctypes.c_uint32 * 1)()
        rc = lib.l5dh_merge_all((ctypes.c_void_p * 1)(eng._ctx.value), 1, int(mode), *ptr, first, count)
        assert rc == 0 and (first[0], count[0]) == (0, S)
        return summ, counts, totals
    want = [case["summ"].tobytes(), case["counts"].tobytes(), case["totals"].tobytes()]
    assert both(eng, case, call, True) == want
