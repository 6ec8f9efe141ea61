"""Scratch lanes (kdb_lane, kdb_internal.h): a lane's buffer that grows while the OTHER lane is the current one.

Two caller streams drive one index alternately through the _dev entry points, so each stream keeps a lane of its own and every
call finds the other stream's lane current when it takes its own.  The schedule makes every buffer of a lane -- prepared queries,
visited bitsets, general scratch, entry points per allow list, the heap-order pass's lists and tails, the by-id decode buffer, and
the work words every walk uses -- grow at least once in each of the two lanes (sizes worked out from the growth rules of
kdb_api.hip: 64 KiB is the smallest scratch, qbuf, tie and by-id buffer, 16 slots the smallest visited set, n + n / 4 + 64 entries a
grown entry-point table).  A buffer that is stored in the wrong lane, freed under the other stream or shared between the two shows
as a wrong answer: every answer of every call must be the oracle's, with the exactness tests/test_gpu_parity.py asks of that
kind of call."""
import numpy as np
import pytest

from conftest import assert_same_results_tol
from test_gpu_parity import build_pair, raw_to_score

pytestmark = pytest.mark.gpu

N, DIM, K, EF = 3000, 32, 10, 50
N_COPIES = 40
SRC = 17   # the row that has the copies (0-based)


def corpus():
    """rows, the 0-based indices of the copies, the deleted ids"""
    rng = np.random.default_rng(23)
    X = rng.standard_normal((N, DIM)).astype(np.float32)
    copies = rng.choice(np.setdiff1d(np.arange(N), [SRC]), N_COPIES, replace=False)
    X[copies] = X[SRC]                                    # forty copies of one row: a heap-order call near it has ties
    deleted = [int(copies[0]) + 1, int(copies[1]) + 1, 5, 900, 2999]
    return X, copies, deleted


def away_from_the_copies(Q, X):
    """Q mirrored onto the far side of the copied row (cosine to it <= 0, where the nearest 50 of 3000 random rows are above 0.3).
    A walk without KDB_SEARCH_HEAP_ORDER orders equal distances by id, the oracle as the reference's heaps hold them: the plain
    calls of this test are compared id for id, so their beams must not hold two copies."""
    c = X[SRC].astype(np.float64) / np.linalg.norm(X[SRC].astype(np.float64))
    d = Q.astype(np.float64) @ c
    return (Q - np.outer(d + np.abs(d), c)).astype(np.float32)


def plain_queries(B, seed, X):
    return away_from_the_copies(np.random.default_rng(seed).standard_normal((B, DIM)).astype(np.float32), X)


def by_id_sources(B, distinct, seed, X, copies, deleted):
    """B source ids drawn from `distinct` stored rows on the far side of the copied row (none of them a copy), the second one deleted"""
    r = np.random.default_rng(seed)
    far = np.nonzero(X @ X[SRC] < 0)[0]
    far = np.setdiff1d(far, np.concatenate([copies, [SRC], np.array(deleted) - 1]))
    pool = (r.choice(far, distinct, replace=False) + 1).astype(np.uint32)
    pool[1] = deleted[2]                                  # a source that is deleted: no results
    src_ids = pool[r.integers(0, distinct, size=B)]
    src_ids[:2] = pool[:2]
    return pool, src_ids


def test_lane_buffers_grow_while_the_other_lane_is_current(oracle, hip):
    import torch
    from kektordb_amd.index import dense_bitset
    O = oracle
    X, copies, deleted = corpus()
    orc, idx = build_pair(O, hip, X, O.COSINE, efc=60, deleted=deleted)
    orc.set_arith(O.ARITH_HIP_WAVE)
    rows = orc.rows()
    TIED = hip.index.COUNT_TIED
    dev = torch.device("cuda:0")
    streams = [torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)]

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    def outputs(B, k):
        return (torch.zeros((B, k), dtype=torch.int32, device=dev), torch.zeros((B, k), dtype=torch.float32, device=dev),
                torch.zeros((B,), dtype=torch.int32, device=dev))

    def host(out):
        oi, od, oc = out
        return oi.cpu().numpy().view(np.uint32), od.cpu().numpy(), oc.cpu().numpy().view(np.uint32)

    def assert_exact(label, b, ids, dist, cnt, want_i, want_d):
        c = int(cnt)
        assert c == len(want_i), (label, b, c, len(want_i))
        assert np.array_equal(ids[:c], want_i), (label, b, ids[:c], want_i)
        assert np.array_equal(raw_to_score(idx, dist[:c]), want_d), (label, b)

    # ---- the kinds of call: each returns (launch(stream) -> outputs, check(label, outputs)); the oracle's answers are made once
    def walk(B, seed, heap=False):
        if heap:   # near the copied row: equal distances inside the beam
            Q = (X[SRC][None, :] + 0.02 * np.random.default_rng(seed).standard_normal((B, DIM))).astype(np.float32)
        else:
            Q = plain_queries(B, seed, X)
        dQ = up(Q)
        want = [orc.search(Q[b], K, ef=EF) for b in range(B)]

        outs = [outputs(B, K) for _ in streams]   # (made here: zero-filled before the synchronize below, not beside the call)

        def launch(s, w):
            out = outs[w]
            idx.search_batch_dev(dQ, K, EF, *out, stream=s, tie_flag=heap, heap_order=heap)
            return out

        def check(label, out):
            ids, dist, cnt = host(out)
            if heap:
                assert not np.any(cnt & TIED), (label, "a tie stayed unresolved")
            for b in range(B):
                assert_exact(label, b, ids[b], dist[b], cnt[b], *want[b])
        return launch, check

    def scan(B, k, seed):
        Q = np.random.default_rng(seed).standard_normal((B, DIM)).astype(np.float32)
        Q[0] = X[SRC]                                     # the cut at k runs through the copies (an exact scan orders by distance, then id)
        dQ = up(Q)
        want = [orc.flat_scan(Q[b], k) for b in range(B)]

        outs = [outputs(B, k) for _ in streams]   # (made here: zero-filled before the synchronize below, not beside the call)

        def launch(s, w):
            out = outs[w]
            idx.flat_scan_batch_dev(dQ, k, *out, stream=s)
            return out

        def check(label, out):
            ids, dist, cnt = host(out)
            for b in range(B):
                c = int(cnt[b])
                assert c == len(want[b][0]), (label, b)
                assert_same_results_tol(ids[b, :c], raw_to_score(idx, dist[b, :c]), *want[b])
                assert_exact(label, b, ids[b], dist[b], cnt[b], *want[b])   # (the wave accumulation order restated in the oracle reproduces the bits)
                assert not (set(ids[b, :c].tolist()) & set(deleted)), (label, b)
        return launch, check

    def multi(G, B, seed):
        r = np.random.default_rng(seed)
        lists = []
        for _ in range(G):
            a = np.nonzero(r.random(N + 1) < 0.3)[0]
            lists.append(dense_bitset(a[a >= 1], N))
        L = np.stack(lists)
        Q = away_from_the_copies(r.standard_normal((B, DIM)).astype(np.float32), X)
        of_q = r.integers(-1, G, size=B).astype(np.int32)  # -1 = no filter
        of_q[:3] = [-1, 0, G - 1]
        dQ, dL, dO = up(Q), up(L.view(np.int64)), up(of_q)
        want = [orc.search(Q[b], K, ef=EF, allow=None if of_q[b] < 0 else L[int(of_q[b])]) for b in range(B)]

        outs = [outputs(B, K) for _ in streams]   # (made here: zero-filled before the synchronize below, not beside the call)

        def launch(s, w):
            out = outs[w]
            idx.search_batch_multi_dev(dQ, K, EF, dL, dO, *out, stream=s)
            return out

        def check(label, out):
            ids, dist, cnt = host(out)
            for b in range(B):
                assert_exact(label, b, ids[b], dist[b], cnt[b], *want[b])
        return launch, check

    def by_id(B, distinct, seed):
        pool, src_ids = by_id_sources(B, distinct, seed, X, copies, deleted)
        d_ids = up(src_ids.view(np.int32))
        gone = set(deleted)
        want = {int(i): orc.search(rows[int(i)], K, ef=EF) for i in pool if int(i) not in gone}

        outs = [outputs(B, K) for _ in streams]   # (made here: zero-filled before the synchronize below, not beside the call)

        def launch(s, w):
            out = outs[w]
            idx.search_by_id_dev(d_ids, K, EF, *out, stream=s)
            return out

        def check(label, out):
            ids, dist, cnt = host(out)
            for b in range(B):
                i = int(src_ids[b])
                if i in gone:
                    assert int(cnt[b]) == 0 and not np.any(ids[b]), (label, b, i)
                else:
                    assert_exact(label, b, ids[b], dist[b], cnt[b], *want[i])
        return launch, check

    # Every step runs once on each stream, the two back to back: call i + 1 goes on the other stream than call i, and each lane
    # meets the small size before the large one.  What grows at a step (in the lane of each stream, the other lane being current):
    schedule = [
        ("walk B=1", walk(1, 1), False),                  # (first buffers: visited 16 slots)
        ("scan k=1 B=1", scan(1, 1, 2), False),           # (scratch and qbuf at their smallest)
        ("multi G=2", multi(2, 12, 3), False),            # (entry points: 66 entries)
        ("heap B=2", walk(2, 4, heap=True), True),        # (tie scratch at its smallest)
        ("by-id B=4", by_id(4, 4, 5), False),             # (by-id buffer at its smallest)
        ("walk B=40", walk(40, 6), False),                # visited 16 -> 64 slots
        ("scan k=200 B=300", scan(300, 200, 7), False),   # scratch (every distance of a chunk of queries), qbuf (512 padded queries)
        ("multi G=130", multi(130, 12, 8), False),        # entry points 66 -> 226
        ("heap B=64", walk(64, 9, heap=True), True),      # tie scratch: 64 workgroups' candidate-heap tails
        ("walk B=3", walk(3, 11), False),                 # (nothing grows: the buffers of a larger call serve a small one)
        ("walk B=300", walk(300, 12), False),             # visited 64 -> 512 slots
        ("by-id B=600", by_id(600, 150, 10), False),      # by-id buffer: 600 decoded rows > 64 KiB; visited 512 -> 1024 slots
    ]
    torch.cuda.synchronize()                              # inputs uploaded and outputs zero-filled (torch's stream) before a caller's stream touches them
    n_heap = 0
    for label, (launch, check), heap in schedule:
        if heap:   # one at a time: the counters of the LAST launch say whether a query took the heap-order pass
            for w, st in enumerate(streams):
                out = launch(st.cuda_stream, w)
                st.synchronize()
                tied = idx.counters()["n_tied"]
                print(f"{label} stream {w}: n_tied {tied}, free HBM {torch.cuda.mem_get_info()[0]}")
                assert tied > 0, (label, w, "no query took the heap-order pass: the case tests nothing")
                check((label, w), out)
                n_heap += 1
            continue
        outs = [launch(st.cuda_stream, w) for w, st in enumerate(streams)]
        for w, st in enumerate(streams):
            st.synchronize()                              # each stream is synchronised before its answers are read
            print(f"{label} stream {w}: free HBM {torch.cuda.mem_get_info()[0]}")
            check((label, w), outs[w])
    assert n_heap == 4
    idx.close()
