"""consensus_host (include/kektor_hip.hpp), the host restatement of kdb_consensus_batch's arithmetic, and the new ABI names.

tests/cpp/consensus_test.cpp compiles with plain g++ against the header and links the shared library, the way test_cpp_by_id.py
compiles its program.  In `host` mode it needs no device: it runs consensus_host on the cases written here and hands the raw results
back, which must equal the numpy restatement (tests/consensus_ref.py) bit for bit -- centroid, every accumulator of the gram matrix,
similarities, score, variance, max_pair: both sides are correctly rounded IEEE arithmetic in the same order.  The four cases of the
reference's TestCalculateConsensus (tests/golden/consensus_kats.json) are checked with that test's own bound.  Without arguments and
without a GPU the program fails loudly (exit 77); on the GPU it checks Index::Consensus / Index::BeliefState against the calls they
replace."""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

from consensus_ref import REC, restate, same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_exe(tmp_path):
    import kektordb_amd
    kektordb_amd.build_library()
    exe = str(tmp_path / "consensus_test")
    libdir = os.path.dirname(kektordb_amd.LIB_PATH)
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "consensus_test.cpp"), "-L", libdir, "-lkektor_hip",
           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-pthread", "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    return exe


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build_exe(tmp_path_factory.mktemp("consensus"))


def run_host(exe, tmp_path, cases):
    """cases: [(rows [n, dim] f32, query [dim] f32 or None)] -> [dict(rec, centroid, similarity, gram)]"""
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for rows, q in cases:
            f.write(struct.pack("<III", rows.shape[0], rows.shape[1], 0 if q is None else 1))
            f.write(np.ascontiguousarray(rows, dtype=np.float32).tobytes())
            if q is not None:
                f.write(np.ascontiguousarray(q, dtype=np.float32).tobytes())
    p = subprocess.run([exe, "host", fin, fout], capture_output=True, text=True)
    assert p.returncode == 0, (p.returncode, p.stdout, p.stderr)
    raw = open(fout, "rb").read()
    out, o = [], 0
    for rows, q in cases:
        n, dim = rows.shape
        r = {"rec": np.frombuffer(raw, dtype=REC, count=1, offset=o)}
        o += 32
        r["centroid"] = np.frombuffer(raw, dtype=np.float32, count=dim, offset=o)
        o += 4 * dim
        r["similarity"] = None
        if q is not None:
            r["similarity"] = np.frombuffer(raw, dtype=np.float64, count=n, offset=o)
            o += 8 * n
        r["gram"] = np.frombuffer(raw, dtype=np.float64, count=(n + 1) * (n + 1), offset=o).reshape(n + 1, n + 1)
        o += 8 * (n + 1) * (n + 1)
        out.append(r)
    assert o == len(raw)
    return out


def want_of(rows, q):
    n, dim = rows.shape
    ones = np.ones((1, n), dtype=bool)
    w = restate(rows[None], ones, ones, None if q is None else q[None])
    return {k: (None if v is None else v[0]) for k, v in w.items()}


def same_where_not_nan(a, b):
    """bit for bit, and NaN exactly where the other has NaN (the sign and payload of a NaN are not arithmetic)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint8), b[~nb].view(np.uint8))


def compare(got, want, has_q, eq=same):
    for f in ("score", "variance", "max_pair"):
        assert eq(got["rec"][f], np.atleast_1d(want["rec"][f])), (f, got["rec"], want["rec"])
    assert int(got["rec"]["n_found"][0]) == int(want["rec"]["n_found"]) and int(got["rec"]["n_active"][0]) == int(want["rec"]["n_active"])
    assert eq(got["centroid"], want["centroid"])
    assert eq(got["gram"], want["gram"])
    if has_q:
        assert eq(got["similarity"], want["similarity"])


def test_consensus_host_equals_the_numpy_restatement(exe, tmp_path):
    rng = np.random.default_rng(5)
    cases = []
    for dim in (3, 100, 772):
        for n in (0, 1, 2, 3, 10, 50, 64):
            rows = rng.standard_normal((n, dim)).astype(np.float32)
            if n >= 3:
                rows[1] += np.float32(3.0) * rows[0]           # not all pairs at the clamp
            cases.append((rows, rng.standard_normal(dim).astype(np.float32) if n % 2 == 0 or n == 1 else None))
    rows = rng.standard_normal((10, 100)).astype(np.float32)
    rows[4] = 0.0                                              # a zero row: distance 1 to everything
    cases.append((rows, rng.standard_normal(100).astype(np.float32)))
    rows = rng.standard_normal((10, 100)).astype(np.float32)
    rows[7] = rows[2]                                          # a duplicated row
    cases.append((rows, rows[2].copy()))
    cases.append((np.repeat(rows[:1], 5, axis=0), None))       # duplicates only: score exactly 1
    cases.append((rng.standard_normal((6, 100)).astype(np.float32), np.zeros(100, dtype=np.float32)))   # a zero query
    n_plain = len(cases)
    rows = rng.standard_normal((10, 100)).astype(np.float32)
    rows[3, 17] = np.nan                                       # a row holding a NaN
    cases.append((rows, rng.standard_normal(100).astype(np.float32)))
    got = run_host(exe, tmp_path, cases)
    for i, ((rows, q), g) in enumerate(zip(cases, got)):
        compare(g, want_of(rows, q), q is not None, same if i < n_plain else same_where_not_nan)
    dup = got[n_plain - 2]
    assert dup["rec"]["score"][0] == 1.0 and dup["rec"]["max_pair"][0] < 1e-10
    nan = got[n_plain]
    assert np.isnan(nan["rec"]["variance"][0]) and np.isnan(nan["similarity"][3]) and not np.isnan(np.delete(nan["similarity"], 3)).any()
    assert not np.isnan(nan["rec"]["max_pair"][0])             # `d > maxVar` is false for a NaN


def test_reference_kats(exe, tmp_path):
    kats = json.load(open(os.path.join(ROOT, "tests", "golden", "consensus_kats.json")))
    tol = kats["tolerance"]
    assert tol == 1e-4 and len(kats["cases"]) == 4
    cases = [(np.array(c["vectors"], dtype=np.float32).reshape(len(c["vectors"]), 3), None) for c in kats["cases"]]
    got = run_host(exe, tmp_path, cases)
    for c, (rows, _), g in zip(kats["cases"], cases, got):
        for r in (g["rec"][0], want_of(rows, None)["rec"]):
            score, var = float(r["score"]), float(r["variance"])
            if c["should_be_near"]:
                assert 0.0 <= score <= 1.0, (c["name"], score)
            else:
                assert abs(score - c["expected_score"]) <= tol and abs(var - c["expected_variance"]) <= tol, (c["name"], score, var)
        if rows.shape[0] == 1:
            assert same(g["centroid"], rows[0])


@pytest.mark.skipif(__import__("conftest").HAS_GPU, reason="CPU-only behaviour")
def test_cpp_consensus_links_and_fails_loudly_without_gpu(exe):
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 77, (p.returncode, p.stdout, p.stderr)
    assert "no CPU fallback" in p.stdout


@pytest.mark.gpu
def test_cpp_consensus_on_gpu(exe):
    # a pure C++ process: the system HIP runtime under /opt/rocm serves it (no torch in this process)
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0, (p.returncode, p.stdout, p.stderr)
    assert "ok" in p.stdout


def test_abi_names_and_record_layout():
    import kektordb_amd
    from kektordb_amd import _lib
    from kektordb_amd.index import CONSENSUS_DTYPE, CONSENSUS_MAX_K
    for name in ("kdb_consensus_batch", "kdb_consensus_batch_dev", "kdb_belief_batch", "kdb_belief_batch_dev"):
        assert name in kektordb_amd.ABI_SYMBOLS
    import ctypes
    assert ctypes.sizeof(_lib.Consensus) == 32 == CONSENSUS_DTYPE.itemsize == REC.itemsize and CONSENSUS_MAX_K == 64
    hdr = open(os.path.join(ROOT, "include", "kektor_hip.h")).read()
    assert "#define KDB_CONSENSUS_MAX_K 64u" in hdr
    for name in ("kdb_consensus_batch", "kdb_consensus_batch_dev", "kdb_belief_batch", "kdb_belief_batch_dev"):
        assert f"KDB_API int {name}(" in hdr
