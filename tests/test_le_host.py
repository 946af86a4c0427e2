"""le_cuts on the host: the snapping of requested `le` bounds to exact cuts
(linkerd_amd/csrc/l5dh_tables.cpp, plain C++) against the CPU oracle under ASan + UBSan,
as a stand-alone program (tests/c/le_check.cpp), and the same function through the
C-ABI (l5dh_le_cuts needs no context and no GPU)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("gcc") is None or shutil.which("g++") is None, reason="gcc / g++ absent")
def test_le_cuts_asan_ubsan(tmp_path):
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    csrc = os.path.join(REPO, "linkerd_amd", "csrc")
    obj, exe = tmp_path / "hist_oracle.o", tmp_path / "le_check"
    cmds = [["gcc", "-O1", "-g", "-std=c11", "-ffp-contract=off", *san, "-c", os.path.join(REPO, "oracle", "hist_oracle.c"),
             "-o", str(obj)],
            ["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", *san, "-I", os.path.join(REPO, "oracle"), "-I", csrc,
             "-o", str(exe), os.path.join(REPO, "tests", "c", "le_check.cpp"), os.path.join(csrc, "l5dh_tables.cpp"),
             str(obj), "-lm", "-lpthread"]]
    for cmd in cmds:
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr[-4000:]
    assert "runtime error" not in r.stderr


@pytest.fixture(scope="module")
def lib():
    from linkerd_amd import _native as N
    if not os.path.exists(N.LIB_PATH):
        if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
            pytest.skip("libl5dhist.so not built and no hipcc to build it")
        subprocess.run(["make", "-s", "-C", os.path.join(REPO, "linkerd_amd", "csrc")], check=True)
    return N.load()


def test_le_cuts_through_the_abi(lib, oracle):
    from linkerd_amd import _native as N
    from linkerd_amd.engine import HistogramEngine
    L = oracle.limits().astype(np.int64)
    bounds = [1, 2, 5, 10, 25, 50, 100, 250, 500, 1000, 60000, float("inf")]
    cuts, le = HistogramEngine.le_cuts(bounds)
    assert cuts.dtype == np.uint32 and le.dtype == np.int64
    assert cuts.tolist() == [2, 3, 6, 11, 26, 51, 101, 193, 262, 332, 743, 1797]
    assert le.tolist() == [1, 2, 5, 10, 25, 50, 100, 250, 497, 997, 59582, int(L[1796]) - 1]
    np.testing.assert_array_equal(le, L[cuts.astype(np.int64) - 1] - 1)
    # brute force over random bounds: c = #{ j : L[j] - 1 <= floor(B) } clipped to [1, 1797]
    rng = np.random.default_rng(11)
    b = np.concatenate([rng.uniform(0, 3e9, 500), rng.uniform(0, 2000, 500)])
    c = np.zeros(b.size, np.uint32)
    assert lib.l5dh_le_cuts(b.ctypes.data, b.size, c.ctypes.data, None) == 0
    want = np.maximum(1, (L[None, :] - 1 <= np.floor(b)[:, None]).sum(axis=1))
    np.testing.assert_array_equal(c, want)
    # duplicates are dropped and the cuts ascend, whatever the order of the bounds
    cuts, le = HistogramEngine.le_cuts([1000, 250, 997, 250.7, 998, 0, 0.5])
    assert cuts.tolist() == [1, 193, 332] and le.tolist() == [0, 250, 997]
    for bad in ([1.0, float("nan")], [-1.0], [5.0, -0.001]):
        with pytest.raises(N.L5dhError) as ei:
            HistogramEngine.le_cuts(bad)
        assert ei.value.code == -22
    assert N.LE_MAX == 64 and "#define L5DH_LE_MAX 64" in open(N.HEADER_PATH).read()
    assert {"l5dh_le", "l5dh_le_dense", "l5dh_le_cuts"} <= set(N.SIGNATURES) & set(N.header_symbols())
