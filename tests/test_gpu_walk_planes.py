"""Walk planes (KDB_INDEX_NO_WALK_PLANES, kdb_index_drop_walk_planes): a float32 cosine index walked in large batches
reads its rows as a plane of high and a plane of low 16-bit halves and rejects, from the high plane alone, candidates it can
PROVE are not nearer than the worst result of a full beam.  The proof is rigorous and survivors are evaluated on the reassembled
float32 values, so nothing a caller can see may change: every comparison here is exact -- ids in order, distance bits, counts, the
tie bit, per-query n_dist and n_hops -- against the oracle's walk (ARITH_HIP_WAVE), and where the oracle has no say (rows that are
not finite) against a second handle created with KDB_INDEX_NO_WALK_PLANES on the same rows and graph.

Batches of 2400 and 8400 queries take the one-wave kernel (the planes kernel); 12 and 480 take the latency modes, which never
read the planes.  Queries are tiled from a few hundred distinct ones: the GPU walks every copy, the oracle each distinct one once."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K = 10
NQ = 300            # distinct queries per corpus
N = 3200            # rows per corpus: more than one visited-hash generation at ef 256, seconds for the oracle


def _clustered(n, dim, seed):
    rng = np.random.default_rng(seed)
    nc = max(4, n // 64)
    cent = rng.standard_normal((nc, dim)).astype(np.float32)
    X = (cent[rng.integers(0, nc, n)] + 0.3 * rng.standard_normal((n, dim))).astype(np.float32)
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    return X.astype(np.float32)


def _queries(X, nq, seed):
    rng = np.random.default_rng(seed)
    return (X[rng.choice(X.shape[0], nq, replace=False)] + 0.05 * rng.standard_normal((nq, X.shape[1]))).astype(np.float32)


def _bits(count, ids):
    w = np.zeros((count >> 6) + 1, dtype=np.uint64)
    for i in ids:
        w[int(i) >> 6] |= np.uint64(1) << np.uint64(int(i) & 63)
    return w


class Pair:
    """one corpus: the index under test (walk planes allowed), the same rows and graph in a handle that opted out, the oracle"""

    def __init__(self, X, deleted=(), efc=100, m=16, extra_cap=0, oracle=True):
        import kektordb_amd as hip
        from oracle import oracle as O
        O.build()
        self.hip, self.O, self.X, self.m, self.efc = hip, O, X, m, efc
        n, dim = X.shape
        self.idx = hip.HipIndex(dim, hip.COSINE, hip.F32, m, efc, capacity=n + extra_cap)
        self.idx.upload_rows(X, 1)
        self.idx.build(n, batch=512, ef_construction=efc, seed=3)
        if len(deleted):
            self.idx.Delete(list(deleted))
        self.deleted = set(int(d) for d in deleted)
        self.graph = self.idx.download_graph()
        self.ref = hip.HipIndex(dim, hip.COSINE, hip.F32, m, efc, capacity=n + extra_cap, walk_planes=False)
        self.ref.upload_rows(X, 1)
        self.ref.upload_graph(*self.graph)
        if len(deleted):
            self.ref.Delete(list(deleted))
        self.orc = self.make_oracle(X) if oracle else None

    def make_oracle(self, X, graph=None, deleted=None):
        O = self.O
        count, entry, max_level, levels, offs, nbrs = graph or self.graph
        rows = np.zeros((count + 1, X.shape[1]), dtype=np.float32)
        rows[1:] = X[:count]
        g = O.Graph(count, levels, max_level, entry, offs, nbrs, _bits(count, self.deleted if deleted is None else deleted))
        orc = O.OracleIndex.from_graph(X.shape[1], O.COSINE, O.F32, self.m, self.efc, rows, g)
        orc.set_arith(O.ARITH_HIP_WAVE)
        return orc


def check_oracle(idx, orc, Q, ef, reps, allow=None, k=K, skip_tied=False, **flags):
    """the GPU's answers to Q tiled `reps` times == the oracle's, query for query (skip_tied: except where KDB_SEARCH_TIE_FLAG
    reports that the fast walk met equal distances -- there the reference's order is its heaps', and the caller compares the
    answer with the opt-out handle's instead)"""
    import kektordb_amd as hip
    want = [orc.search(Q[b], k, allow=allow, ef=ef, counters=True) for b in range(Q.shape[0])]
    ids, dist, cnt, (nd, nh) = idx.search_batch(np.tile(Q, (reps, 1)), k, ef, allow_bits=allow, trace=True, **flags)
    tied = (cnt & hip.index.COUNT_TIED) != 0
    assert skip_tied or not tied.any()
    assert tied.sum() < tied.size, "every query ties: the case compares nothing"
    for b in range(ids.shape[0]):
        if tied[b]:
            continue
        oi, od, (ond, onh) = want[b % Q.shape[0]]
        c = int(cnt[b])
        assert c == len(oi), (ef, b, c, len(oi))
        assert np.array_equal(ids[b, :c], oi), (ef, b, ids[b, :c], oi)
        assert np.array_equal(1.0 - dist[b, :c].astype(np.float64), od), (ef, b)
        assert (int(nd[b]), int(nh[b])) == (ond, onh), (ef, b, int(nd[b]), int(nh[b]), ond, onh)


def check_same(a, b, Q, ef, k=K, allow=None, **flags):
    """two handles, the same batch: every output array equal bit for bit (the tie bit included), and the counters"""
    ra = a.search_batch(Q, k, ef, allow_bits=allow, trace=True, tie_flag=True, **flags)
    rb = b.search_batch(Q, k, ef, allow_bits=allow, trace=True, tie_flag=True, **flags)
    assert np.array_equal(ra[0], rb[0]), ef
    assert np.array_equal(ra[1].view(np.uint32), rb[1].view(np.uint32)), ef
    assert np.array_equal(ra[2], rb[2]), ef
    assert np.array_equal(ra[3][0], rb[3][0]) and np.array_equal(ra[3][1], rb[3][1]), ef
    return ra


@functools.lru_cache(maxsize=None)
def _pair(dim):
    return Pair(_clustered(N, dim, seed=dim)), _queries(_clustered(N, dim, seed=dim), NQ, seed=dim + 1)


@functools.lru_cache(maxsize=None)
def _pair_deleted():
    X = _clustered(N, 768, seed=5)
    rng = np.random.default_rng(6)
    return Pair(X, deleted=rng.choice(np.arange(1, N + 1), N // 10, replace=False)), _queries(X, NQ, seed=7)


def _free():
    import torch
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


# ---- parity ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ef", [10, 24, 60, 64, 100, 128, 200, 256])   # every register beam: one, two and four slots of 64 entries
def test_parity_768_every_register_beam(ef):
    p, Q = _pair(768)
    check_oracle(p.idx, p.orc, Q, ef, reps=8)                            # 2400 queries: the one-wave kernel


def test_parity_768_lds_beam_is_untouched():
    """ef 300 walks with the LDS beam: its large batches do not read the planes (this version); answers as ever"""
    p, Q = _pair(768)
    check_oracle(p.idx, p.orc, Q[:150], 300, reps=16)


@pytest.mark.parametrize("reps,nq", [(28, 300), (1, 12), (2, 240)])     # 8400 queries: one wave; 12 and 480: the latency modes
def test_parity_768_other_batch_sizes(reps, nq):
    p, Q = _pair(768)
    check_oracle(p.idx, p.orc, Q[:nq], 60, reps=reps)


@pytest.mark.parametrize("dim", [384, 128])
@pytest.mark.parametrize("ef", [24, 60, 200])
def test_parity_other_widths_walk_as_before(dim, ef):
    """384 and 128 columns do not get planes in this version: their large batches answer as before"""
    p, Q = _pair(dim)
    check_oracle(p.idx, p.orc, Q, ef, reps=8)


@pytest.mark.parametrize("ef", [24, 60, 128])
def test_parity_deleted_nodes(ef):
    p, Q = _pair_deleted()
    check_oracle(p.idx, p.orc, Q, ef, reps=8)


@pytest.mark.parametrize("share", [0.5, 0.1])
@pytest.mark.parametrize("ef", [24, 100])
def test_parity_allow_lists(share, ef):
    p, Q = _pair(768)
    rng = np.random.default_rng(int(share * 100))
    allow = _bits(N, rng.choice(np.arange(1, N + 1), int(N * share), replace=False))
    check_oracle(p.idx, p.orc, Q, ef, reps=8, allow=allow)


@pytest.mark.parametrize("ef", [24, 60, 200])
def test_parity_tie_and_heap_order_flags(ef):
    p, Q = _pair(768)
    Qt = np.tile(Q, (8, 1))
    check_oracle(p.idx, p.orc, Q, ef, reps=8, tie_flag=True, skip_tied=True)       # (near-orthogonal dots mark a walk as tied)
    check_oracle(p.idx, p.orc, Q, ef, reps=8, tie_flag=True, heap_order=True)      # heap order resolves every tie
    check_same(p.idx, p.ref, Qt, ef)
    check_same(p.idx, p.ref, Qt, ef, heap_order=True)


# ---- the bound, adversarial ----------------------------------------------------------------------------------------------------------
def _low_bits_family(dim, seed):
    """rows that differ from one another only in the low 16 bits of their components: blocks of 64 rows share one high plane, so
    whole blocks sit within `err` of each other -- and of the worst result"""
    rng = np.random.default_rng(seed)
    base = _clustered(N // 64, dim, seed)
    X = np.repeat(base, 64, axis=0)
    bits = X.view(np.uint32) & np.uint32(0xffff0000)
    X = (bits | rng.integers(0, 1 << 16, X.shape, dtype=np.uint32)).view(np.float32)
    return np.ascontiguousarray(X[rng.permutation(X.shape[0])])


@pytest.mark.parametrize("ef", [10, 60, 128])
def test_bound_rows_that_share_their_high_plane(ef):
    """(dots of such rows often round to the SAME float: the fast walk orders equal distances by id, the reference by its heaps'
    history -- so the oracle is compared under KDB_SEARCH_HEAP_ORDER, and without it wherever the tie flag stays clear; the opt-out
    handle must agree bit for bit either way)"""
    X = _low_bits_family(768, seed=31)
    p = Pair(X)
    Q = _queries(X, 150, seed=32)
    check_oracle(p.idx, p.orc, Q, ef, reps=16, tie_flag=True, heap_order=True)
    check_oracle(p.idx, p.orc, Q, ef, reps=16, tie_flag=True, skip_tied=True)
    check_same(p.idx, p.ref, np.tile(Q, (16, 1)), ef)


def test_bound_duplicates_of_the_worst_result_stay_rejected():
    """48 exact copies of one row around every query: keys EQUAL to the worst result are met at every hop (key == worst does not
    pass).  Ties: the oracle's heap order is compared under KDB_SEARCH_HEAP_ORDER, the fast walk against the opt-out handle"""
    import kektordb_amd as hip
    rng = np.random.default_rng(41)
    X = _clustered(N, 768, seed=40)
    base = X[7].copy()
    X[rng.choice(N, 48, replace=False)] = base[None, :]
    Q = (base[None, :] + 0.02 * rng.standard_normal((40, 768))).astype(np.float32)
    p = Pair(X)
    Qt = np.tile(Q, (60, 1))
    for ef in (20, 40, 100):
        want = [p.orc.search(Q[b], K, ef=ef, counters=True) for b in range(Q.shape[0])]
        ids, dist, cnt, (nd, nh) = p.idx.search_batch(Qt, K, ef, trace=True, tie_flag=True, heap_order=True)
        assert not np.any(cnt & hip.index.COUNT_TIED)
        for b in range(Qt.shape[0]):
            oi, od, (ond, onh) = want[b % Q.shape[0]]
            c = int(cnt[b])
            assert c == len(oi) and np.array_equal(ids[b, :c], oi), (ef, b)
            assert np.array_equal(1.0 - dist[b, :c].astype(np.float64), od), (ef, b)
            assert (int(nd[b]), int(nh[b])) == (ond, onh), (ef, b)
        got = check_same(p.idx, p.ref, Qt, ef)
        assert np.any(got[2] & hip.index.COUNT_TIED), "no walk met equal distances: the case tests nothing"


@pytest.mark.parametrize("ef", [24, 100])
def test_bound_mixed_norms_denormals_and_zero_rows(ef):
    """rows of norm 1e-3, 1 and 1e3 in one index, rows whose components are denormal or -0, all-zero rows"""
    rng = np.random.default_rng(51)
    X = _clustered(N, 768, seed=50)
    X *= rng.choice(np.array([1e-3, 1.0, 1e3], dtype=np.float32), N)[:, None]
    tiny = rng.choice(N, 60, replace=False)
    X[tiny[:20]] = (rng.integers(0, 1 << 20, (20, 768), dtype=np.uint32) | (rng.integers(0, 2, (20, 768), dtype=np.uint32) << 31)).view(np.float32)  # denormals
    X[tiny[20:40]] = 0.0
    X[tiny[40:]] = -0.0
    X[tiny[40:], :5] = 1e-3
    p = Pair(np.ascontiguousarray(X))
    Q = _queries(_clustered(N, 768, seed=50), 150, seed=52)
    check_same(p.idx, p.ref, np.tile(Q, (16, 1)), ef)
    import kektordb_amd as hip
    want = [p.orc.search(Q[b], K, ef=ef, counters=True) for b in range(Q.shape[0])]
    ids, dist, cnt, (nd, nh) = p.idx.search_batch(np.tile(Q, (16, 1)), K, ef, trace=True, tie_flag=True)
    for b in range(ids.shape[0]):
        if cnt[b] & hip.index.COUNT_TIED:                                # (zero rows: equal distances; the opt-out handle agreed above)
            continue
        oi, od, (ond, onh) = want[b % Q.shape[0]]
        c = int(cnt[b])
        assert c == len(oi) and np.array_equal(ids[b, :c], oi), (ef, b)
        assert np.array_equal(1.0 - dist[b, :c].astype(np.float64), od), (ef, b)
        assert (int(nd[b]), int(nh[b])) == (ond, onh), (ef, b)


@pytest.mark.parametrize("ef", [24, 100])
def test_bound_rows_that_are_not_finite(ef):
    """a few rows holding NaN, +-Inf or 3e38: no fault, and answers identical to the handle without planes"""
    rng = np.random.default_rng(61)
    X = _clustered(N, 768, seed=60)
    p0 = Pair(X, oracle=False)                                          # the graph of the clean rows
    bad = rng.choice(N, 24, replace=False)
    Xb = X.copy()
    Xb[bad[:6], 3] = np.nan
    Xb[bad[6:12], 700] = np.inf
    Xb[bad[12:18], 0] = -np.inf
    Xb[bad[18:], ::7] = 3e38
    Q = np.tile(_queries(X, 150, seed=62), (16, 1))
    check_same(p0.idx, p0.ref, Q, ef)                                    # the planes exist: the uploads below convert their own rows
    for i in bad:                                                        # (one by one: overwrites of single rows)
        p0.idx.upload_rows(Xb[i:i + 1], int(i) + 1)
        p0.ref.upload_rows(Xb[i:i + 1], int(i) + 1)
    check_same(p0.idx, p0.ref, Q, ef)
    check_same(p0.idx, p0.ref, Q, ef, heap_order=True)
    p0.idx.drop_walk_planes()                                            # ... and planes made from the bad rows
    check_same(p0.idx, p0.ref, Q, ef)


# ---- lifecycle -------------------------------------------------------------------------------------------------------------------------
def test_lifecycle_every_writer_of_rows_keeps_the_planes_current():
    rng = np.random.default_rng(71)
    dim, n0, n1 = 768, 2400, 2800
    Xall = _clustered(n1, dim, seed=70)
    p = Pair(Xall[:n0].copy(), extra_cap=n1 - n0)
    Q = _queries(Xall, 150, seed=72)
    X = Xall[:n0].copy()
    check_oracle(p.idx, p.orc, Q, 60, reps=16)                           # the planes exist from here on
    # 1. overwrite rows that are current results (and their neighbours): the graph stays, the rows move
    ids, _, _ = p.idx.search_batch(Q[:40], K, 60)
    hit = np.unique(ids[ids > 0])[:200]
    X[hit - 1] = _clustered(hit.size, dim, seed=73)
    p.idx.upload_rows(X[hit.min() - 1:hit.max()], int(hit.min()))         # one range upload ...
    p.idx.upload_rows(X[hit[0] - 1:hit[0]], int(hit[0]))                  # ... and a single row
    check_oracle(p.idx, p.make_oracle(X), Q, 60, reps=16)
    # 2. append rows, link them, raise the count
    levels = np.zeros(n1 - n0, dtype=np.uint8)
    p.idx.upload_rows(Xall[n0:n1], n0 + 1)
    p.idx.add_batch(n0 + 1, levels, ef_construction=100)
    X = np.concatenate([X, Xall[n0:n1]])
    g = p.idx.download_graph()
    assert g[0] == n1
    check_oracle(p.idx, p.make_oracle(X, graph=g), Q, 60, reps=16)
    # 3. reserve: every per-id array moves, the planes with them
    p.idx.reserve(2 * n1)
    check_oracle(p.idx, p.make_oracle(X, graph=g), Q, 60, reps=16)
    check_oracle(p.idx, p.make_oracle(X, graph=g), Q, 200, reps=16)
    # 4. vacuum: deleted rows are cleared, in the planes too
    dead = rng.choice(np.arange(1, n1 + 1), 150, replace=False)
    p.idx.Delete([int(d) for d in dead])
    p.idx.vacuum(ef_construction=100)
    g = p.idx.download_graph()
    X[dead - 1] = 0.0
    check_oracle(p.idx, p.make_oracle(X, graph=g, deleted=dead), Q, 60, reps=16)
    # 5. drop: the next large walk makes them again; refused for good: device memory stays flat
    free_with = _free()
    p.idx.drop_walk_planes()
    planes = 2 * (2 * n1 + 1) * dim * 2
    assert _free() - free_with >= planes * 3 // 4
    check_oracle(p.idx, p.make_oracle(X, graph=g, deleted=dead), Q, 60, reps=16)
    assert _free() <= free_with + planes // 4
    p.idx.drop_walk_planes(refuse_for_good=True)
    free_without = _free()
    check_oracle(p.idx, p.make_oracle(X, graph=g, deleted=dead), Q, 60, reps=16)
    assert free_without - _free() < planes // 4


# ---- allocation ------------------------------------------------------------------------------------------------------------------------
def test_allocation_small_walks_and_l2_indexes_leave_device_memory_alone():
    import kektordb_amd as hip
    dim, n = 768, N
    X = _clustered(n, dim, seed=80)
    Q = _queries(X, 300, seed=81)
    planes = 2 * (4 * n + 1) * dim * 2                                   # (sized by the capacity: 39 MB, well above allocation granules)
    idx = hip.HipIndex(dim, hip.COSINE, hip.F32, 16, 100, capacity=4 * n)
    idx.upload_rows(X, 1)
    idx.build(n, batch=512, ef_construction=100, seed=3)
    idx.search_batch(np.tile(Q, (8, 1)), K, 300)                          # (scratch of a large batch, without planes: the LDS beam)
    idx.search_batch(Q[:64], K, 60)
    free0 = _free()
    idx.search_batch(Q[:64], K, 60)                                      # a 64-query walk: latency mode
    assert free0 - _free() < planes // 4
    idx.search_batch(np.tile(Q, (8, 1)), K, 60)                           # 2400 queries: the planes, once
    free1 = _free()
    assert free0 - free1 >= planes
    idx.search_batch(np.tile(Q, (8, 1)), K, 60)
    idx.search_batch(np.tile(Q, (8, 1)), K, 24)
    assert free1 - _free() < planes // 4
    idx.close()
    l2 = hip.HipIndex(dim, hip.L2, hip.F32, 16, 100, capacity=4 * n)
    l2.upload_rows(X, 1)
    l2.build(n, batch=512, ef_construction=100, seed=3)
    l2.search_batch(Q[:64], K, 60)
    l2.search_batch(np.tile(Q, (8, 1)), K, 300)
    free0 = _free()
    l2.search_batch(np.tile(Q, (8, 1)), K, 60)
    assert free0 - _free() < planes // 4
    l2.close()
