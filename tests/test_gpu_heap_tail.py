"""The heap-order walk (heap_walk_kernel, kektordb_amd/csrc/search_heap.hip) where its candidate heap leaves LDS: the HBM tail behind
the first nl_c entries, and the overflow branch behind cap_c entries.

The reference's candidate heap is only that long when the result set cannot fill: on an index whose nodes are almost all
soft-deleted (deleted neighbours are pushed as candidates and never become results) -- its ordinary state between Delete and Vacuum.
With duplicate rows in it the fast walk ties and the query is walked again in heap order; tests/heap_tail_ref.py builds such corpora
(the oracle builds the graph, both sides hold it).  No other corpus of the suite that ties has more than a tenth of its nodes deleted,
so none reaches the tail accessors of HeapStore, the `all` switch of the vectorised sifts at the LDS/HBM border, the g_lo word of
int8 keys, VisHash::migrate inside the pass, or the `over` branch with heap_restore_stashed.

Every case takes a census on the CPU before it compares anything, from the index's own plan (HipIndex.heap_plan: nl_c, cap_c),
the oracle's level-0 candidate-heap peak of every query (OracleIndex.last_peak_candidates) and the tie flags of one fast walk:
a query is "in the tail" when it ties and its peak is above nl_c and at most cap_c, "over" when it ties and its peak is above
cap_c.  The shapes were settled with the oracle alone; the figures behind each cell are in CELLS."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import heap_tail_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 10
REPS = 200            # 24 queries tiled to 4800: the pass runs beside the search kernel from 4096 queries on
TIED = np.uint32(0x80000000)

# name -> rows, columns, metric, precision, share of the nodes below the top level deleted, ef, dist64
# (peaks: the oracle's level-0 candidate-heap peak over the 24 queries, min / max, against the plan's nl_c / cap_c)
CELLS = {
    "f32-l2-ef60": (3000, 32, R.L2, R.F32, 0.96, 60, False),        # nl_c 1330, cap_c 2048, peaks 1352 / 1593; register result heap
    "f32-cos-ef60": (3000, 32, R.COSINE, R.F32, 0.96, 60, False),   # nl_c 1330, cap_c 2048, peaks 1419 / 1610; 1.0 - float64(dot) keys
    "f32-l2-ef200": (4500, 32, R.L2, R.F32, 0.96, 200, False),      # nl_c 2524, cap_c 3200, peaks 2911 / 3040; 4096-word hash, LDS result heap
    "f32-l2-ef300": (7000, 32, R.L2, R.F32, 0.95, 300, False),      # nl_c 2537, cap_c 4800, peaks 4353 / 4518; HBM bitset (at 0.96 fewer
                                                                    # than 300 nodes live: the result set never fills, the walk visits all)
    "f16-l2-ef60": (3000, 32, R.L2, R.F16, 0.96, 60, False),        # nl_c 1330, cap_c 2048, peaks 1372 / 1602
    "i8-cos-ef70": (3000, 32, R.COSINE, R.I8, 0.96, 70, True),      # nl_c 770, cap_c 2048, peaks 1530 / 1741; three-word entries, the g_lo tail
    "f32-cos-768-ef60": (3000, 768, R.COSINE, R.F32, 0.96, 60, False),  # nl_c 962, cap_c 2048, peaks 1556 / 1717; NCH = 12
    # overflow: some walks outgrow cap_c, others stay in the tail, in one launch
    "over-f32-l2-ef60": (9000, 32, R.L2, R.F32, 0.96, 60, False),   # nl_c 1330, cap_c 2048, peaks 1734 / 2389: 15 in the tail, 9 over
    "over-i8-cos-ef70": (6000, 32, R.COSINE, R.I8, 0.96, 70, True), # nl_c 770, cap_c 2048, peaks 1774 / 2303: 14 in the tail, 10 over
    # clipped: cap_c = count + 2, no walk can overflow
    "clipped-i8-cos-ef70": (2000, 32, R.COSINE, R.I8, 0.96, 70, True),  # nl_c 770, cap_c 2002, peaks 1309 / 1408
}
HASH_LIMIT = 2048 - 256 - 64      # VisHash::begin_layer: beyond it the 2048-word hash migrates to the bitset


@functools.lru_cache(maxsize=None)
def corpus(name):
    """-> (the corpus with its oracle, the index under test holding the oracle's rows and graph): built once per module"""
    import kektordb_amd as hip
    from oracle import oracle as O
    O.build()
    n, dim, metric, prec, share, ef, dist64 = CELLS[name]
    c = R.TailCorpus(O, n, dim, metric, prec, share, seed=5)
    idx = hip.HipIndex(dim, metric, prec, R.M, R.EFC, capacity=n + 8)
    idx.upload_rows(c.orc.rows()[1:], 1)
    if prec == R.I8:
        idx.upload_norms(c.orc.norms()[1:], 1)
        idx.set_quantizer(c.orc.absmax)
    idx.upload_graph_obj(c.graph)
    return c, idx


def census(name, B=R.NQ):
    """-> (plan, peaks[24], tied[24], in_tail[24], over[24]); what the fast walk answers without heap order comes along"""
    c, idx = corpus(name)
    ef, dist64 = CELLS[name][5], CELLS[name][6]
    plan = idx.heap_plan(K, ef, B)
    peaks = np.array([w[3] for w in c.want(K, ef)])
    plain = idx.search_batch(c.Q, K, ef, trace=True, tie_flag=True, dist64=dist64)
    plain_dropped = idx.counters()["n_dropped"]
    tied = (plain[2] & TIED) != 0
    in_tail = tied & (peaks > plan["nl_c"]) & (peaks <= plan["cap_c"])
    over = tied & (peaks > plan["cap_c"])
    print(f"{name}: nl_c {plan['nl_c']} cap_c {plan['cap_c']} lds {plan['lds_bytes']} grid {plan['grid']} tied {int(tied.sum())} "
          f"in the tail {int(in_tail.sum())} over {int(over.sum())} peaks {peaks.min()} / {peaks.max()} fast walk dropped {plain_dropped}")
    return plan, peaks, tied, in_tail, over, plain, plain_dropped


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def assert_oracle(name, res, which):
    """queries `which` of a 24-query answer: ids in order, distance bits, count, n_dist, n_hops of the oracle, no tie bit"""
    c, idx = corpus(name)
    ef = CELLS[name][5]
    ids, dist, cnt, (nd, nh) = res
    want = c.want(K, ef)
    for b in np.flatnonzero(which):
        oi, od, (ond, onh), _ = want[b]
        assert not (cnt[b] & TIED), (name, b)
        n = int(cnt[b])
        assert n == len(oi), (name, b, n, len(oi))
        assert np.array_equal(ids[b, :n], oi), (name, b, ids[b, :n], oi)
        assert same_bits(np.array([idx.score(r) for r in dist[b, :n]], dtype=np.float64), od), (name, b)
        assert (int(nd[b]), int(nh[b])) == (ond, onh), (name, b, int(nd[b]), int(nh[b]), ond, onh)


def assert_same_answers(name, got, want, reps):
    """a tiled answer against the 24-query answer, bit for bit, per-query counters included"""
    assert np.array_equal(got[0], np.tile(want[0], (reps, 1))), name
    assert same_bits(got[1], np.tile(want[1], (reps, 1))), name
    assert np.array_equal(got[2], np.tile(want[2], reps)), name
    assert np.array_equal(got[3][0], np.tile(want[3][0], reps)) and np.array_equal(got[3][1], np.tile(want[3][1], reps)), name


def heap_order(name, reps=1, **kw):
    c, idx = corpus(name)
    ef, dist64 = CELLS[name][5], CELLS[name][6]
    Q = c.Q if reps == 1 else np.tile(c.Q, (reps, 1))
    res = idx.search_batch(Q, K, ef, trace=True, tie_flag=True, heap_order=True, dist64=dist64, **kw)
    return res, idx.counters(), idx.launch_shape()[0]


@functools.lru_cache(maxsize=None)
def alone(name):
    """the 24 queries alone (the pass behind the kernel): computed once, shared, never modified"""
    return heap_order(name)


def run_sweep_child(name, tmp_path):
    """the 24 queries alone and tiled in a process whose pass beside the kernel walks nothing (KDB_HEAP_OVERLAP_GIVE_UP is read once
    per process): the sweep behind it walks every tied query -> what that process saw"""
    out = str(tmp_path / "sweep.npz")
    code = f"import sys; sys.path[:0] = [{ROOT!r}, {os.path.join(ROOT, 'tests')!r}]; import test_gpu_heap_tail as T; T.sweep_child({name!r}, {out!r})"
    env = dict(os.environ, KDB_HEAP_OVERLAP_GIVE_UP="1")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0 and "sweep done" in r.stdout, (r.stdout[-500:], r.stderr[-1500:])
    z = np.load(out)
    unpack = lambda p: (z[p + "ids"], z[p + "dist"], z[p + "cnt"], (z[p + "nd"], z[p + "nh"]))
    return unpack("a_"), unpack("t_"), json.loads(str(z["meta"]))


def sweep_child(name, out):
    c, idx = corpus(name)
    ef, dist64 = CELLS[name][5], CELLS[name][6]
    a, _, _ = heap_order(name)
    idx.search_batch(np.tile(c.Q, (REPS, 1)), K, ef, trace=True, tie_flag=True, dist64=dist64)
    plain_dropped = idx.counters()["n_dropped"]
    t, ctr, shape = heap_order(name, REPS)
    pack = lambda p, r: {p + "ids": r[0], p + "dist": r[1], p + "cnt": r[2], p + "nd": r[3][0], p + "nh": r[3][1]}
    np.savez(out, meta=json.dumps({"ctr": ctr, "shape": shape, "plain_dropped": plain_dropped}), **pack("a_", a), **pack("t_", t))
    print("sweep done")


# ---- the tail ------------------------------------------------------------------------------------------------------------------------
TAIL_CELLS = ["f32-l2-ef60", "f32-cos-ef60", "f32-l2-ef200", "f32-l2-ef300", "f16-l2-ef60", "i8-cos-ef70", "f32-cos-768-ef60"]
MODE_CELLS = ["f32-l2-ef60", "i8-cos-ef70"]


def tail_census(name):
    plan, peaks, tied, in_tail, over, _, _ = census(name)
    assert in_tail.sum() >= 8 and not over.any(), (name, plan, int(in_tail.sum()), int(over.sum()), peaks)
    n, dim, metric, prec, share, ef, dist64 = CELLS[name]
    # the instantiation the cell was written for
    assert plan["hash_words"] == (2048 if ef <= 100 else 4096 if ef <= 260 else 0), plan
    assert plan["reg_results"] == (1 if ef <= 62 else 0), plan
    assert plan["nl_c"] < plan["cap_c"] < n + 2, plan
    return tied


@pytest.mark.parametrize("name", TAIL_CELLS)
def test_tail_parity(name):
    """every tied walk's candidate heap reaches into the HBM tail and none outgrows it: every answer is the oracle's"""
    tied = tail_census(name)
    c, idx = corpus(name)
    ef = CELLS[name][5]
    if name == "f32-l2-ef60":   # ... and the 2048-word hash fills in the middle of the heap pass (VisHash::migrate)
        visited = [R.restated_walk(c, b, K, ef)[3] for b in range(R.NQ)]
        assert sum(v > HASH_LIMIT for v in visited) >= 8, visited
    res, ctr, shape = alone(name)
    assert shape["heap_pass"] == 1 and shape["heap_overlap"] == 0, shape
    assert shape["heap_nch"] == (12 if CELLS[name][1] == 768 else 0), shape
    assert_oracle(name, res, np.ones(R.NQ, dtype=bool))
    assert ctr["n_dropped"] == 0 and ctr["n_tied"] == int(tied.sum()) > 0, ctr


@pytest.mark.parametrize("name", MODE_CELLS)
def test_tail_parity_pass_beside_the_kernel(name):
    tied = tail_census(name)
    res, ctr, shape = heap_order(name, REPS)
    assert shape["heap_pass"] == 1 and shape["heap_overlap"] == 1, shape
    assert_same_answers(name, res, alone(name)[0], REPS)
    assert ctr["n_dropped"] == 0 and ctr["n_tied"] == REPS * int(tied.sum()), ctr


@pytest.mark.parametrize("name", MODE_CELLS)
def test_tail_parity_sweep(name, tmp_path):
    tied = tail_census(name)
    a, t, meta = run_sweep_child(name, tmp_path)
    assert meta["shape"]["heap_overlap"] == 1, meta
    want = alone(name)[0]
    assert_same_answers(name, a, want, 1)
    assert_same_answers(name, t, want, REPS)
    assert meta["ctr"]["n_dropped"] == 0 and meta["ctr"]["n_tied"] == REPS * int(tied.sum()), meta


def test_clipped_capacity_cannot_overflow():
    """at most 2046 rows: cap_c = count + 2, a heap never holds more entries than there are nodes"""
    name = "clipped-i8-cos-ef70"
    plan, peaks, tied, in_tail, over, _, _ = census(name)
    n = CELLS[name][0]
    assert n <= 2046 and plan["cap_c"] == n + 2, plan
    assert in_tail.sum() >= 8 and not over.any(), (plan, int(in_tail.sum()), peaks)
    res, ctr, shape = alone(name)
    assert_oracle(name, res, np.ones(R.NQ, dtype=bool))       # every tie resolved
    assert ctr["n_dropped"] == 0 and ctr["n_tied"] == int(tied.sum()) > 0, ctr


# ---- overflow ------------------------------------------------------------------------------------------------------------------------
OVER_CELLS = ["over-f32-l2-ef60", "over-i8-cos-ef70"]


def over_census(name):
    plan, peaks, tied, in_tail, over, plain, plain_dropped = census(name)
    assert over.sum() >= 4 and in_tail.sum() >= 4, (name, plan, int(over.sum()), int(in_tail.sum()), peaks)
    return tied, over, plain, plain_dropped


def assert_over(name, res, tied, over, plain):
    """a 24-query answer of a launch in which some walks outgrow cap_c"""
    assert_oracle(name, res, tied & ~over)                      # in the tail or below it: the oracle's
    keep = over | ~tied                                         # over: the fast walk's answer stays, and so does the tie bit
    assert ((res[2][over] & TIED) != 0).all(), (name, res[2][over])
    assert np.array_equal(res[0][keep], plain[0][keep]) and same_bits(res[1][keep], plain[1][keep]), name
    assert np.array_equal(res[2][keep], plain[2][keep]), name
    assert np.array_equal(res[3][0][keep], plain[3][0][keep]) and np.array_equal(res[3][1][keep], plain[3][1][keep]), name


@pytest.mark.parametrize("name", OVER_CELLS)
def test_overflow_keeps_the_fast_walks_answer(name):
    tied, over, plain, plain_dropped = over_census(name)
    c, idx = corpus(name)
    ef, dist64 = CELLS[name][5], CELLS[name][6]
    res, ctr, shape = alone(name)
    assert shape["heap_pass"] == 1 and shape["heap_overlap"] == 0, shape
    assert_over(name, res, tied, over, plain)
    assert ctr["n_dropped"] - plain_dropped == int(over.sum()), (ctr, plain_dropped)
    # KDB_SEARCH_FAIL_ON_DROP on the host-pointer call: status -7, the outputs delivered all the same
    import ctypes as C
    from kektordb_amd.index import SEARCH_DIST_F64, SEARCH_HEAP_ORDER, SEARCH_TIE_FLAG
    q = np.ascontiguousarray(c.Q, dtype=np.float32)
    ids = np.zeros((R.NQ, K), dtype=np.uint32)
    dist = np.full((R.NQ, K), np.inf, dtype=np.float64 if dist64 else np.float32)
    cnt = np.zeros(R.NQ, dtype=np.uint32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = idx.L.kdb_search_batch(idx.h, ptr(q), R.NQ, K, ef, None, idx._flags() | 4 | (SEARCH_DIST_F64 if dist64 else 0) | SEARCH_TIE_FLAG | SEARCH_HEAP_ORDER,
                                ptr(ids), ptr(dist), ptr(cnt))
    assert rc == -7, rc
    assert np.array_equal(ids, res[0]) and same_bits(dist, res[1]) and np.array_equal(cnt, res[2]), name


@pytest.mark.parametrize("name", OVER_CELLS)
def test_overflow_pass_beside_the_kernel_restores_the_stash(name):
    tied, over, plain, _ = over_census(name)
    c, idx = corpus(name)
    ef, dist64 = CELLS[name][5], CELLS[name][6]
    idx.search_batch(np.tile(c.Q, (REPS, 1)), K, ef, trace=True, tie_flag=True, dist64=dist64)
    plain_dropped = idx.counters()["n_dropped"]
    res, ctr, shape = heap_order(name, REPS)
    assert shape["heap_pass"] == 1 and shape["heap_overlap"] == 1, shape
    want = alone(name)[0]
    assert_over(name, want, tied, over, plain)
    assert_same_answers(name, res, want, REPS)
    assert ctr["n_dropped"] - plain_dropped == REPS * int(over.sum()), (ctr, plain_dropped)


@pytest.mark.parametrize("name", OVER_CELLS)
def test_overflow_sweep_restores_the_stash(name, tmp_path):
    tied, over, plain, _ = over_census(name)
    a, t, meta = run_sweep_child(name, tmp_path)
    assert meta["shape"]["heap_overlap"] == 1, meta
    want = alone(name)[0]
    assert_over(name, want, tied, over, plain)
    assert_same_answers(name, a, want, 1)
    assert_same_answers(name, t, want, REPS)
    assert meta["ctr"]["n_dropped"] - meta["plain_dropped"] == REPS * int(over.sum()), meta
