"""The planes walk at three waves per SIMD: hnsw_search_kernel<f32, cosine, 768 columns, one-slot beam, planes> is
compiled for twelve resident walks per CU instead of eight.  Nothing a caller can see may change.  8400 queries are more than one
round of twelve walks on every CU (LDS and visited state are reused by a second walk) and take the one-wave kernel; ef 24, 60 and
64 are the one-slot beam.  Every comparison is exact -- ids in order, distance bits, counts, the tie bit, per-query n_dist and
n_hops -- against a handle whose planes were dropped for good (kdb_index_drop_walk_planes: the float32 rows, two waves per SIMD)
and against the oracle's walk.  The corpus must exercise every trip shape of compute_dists: hops with 1-4, 5-8, 9-16 and more than
16 new neighbours (one one-row trip, one two-row trip, two trips, three and more) -- asserted on the CPU from a restatement of the
level-0 loop that is itself checked against the oracle."""
import ctypes as C
import functools
import heapq

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K = 10
N = 6000
NQ = 300
REPS = 28           # 8400 queries
EFS = [24, 60, 64]


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


class Corpus:
    """the index under test, the same rows and graph in a handle whose planes are dropped for good, the oracle, the queries"""

    def __init__(self, seed, deleted=()):
        import kektordb_amd as hip
        from oracle import oracle as O
        O.build()
        self.X = X = _clustered(N, 768, seed)
        self.Q = _queries(X, NQ, seed + 1)
        self.Qt = np.tile(self.Q, (REPS, 1))
        self.idx = hip.HipIndex(768, hip.COSINE, hip.F32, 16, 100, capacity=N)
        self.idx.upload_rows(X, 1)
        self.idx.build(N, batch=512, ef_construction=100, seed=3)
        self.graph = self.idx.download_graph()
        self.ref = hip.HipIndex(768, hip.COSINE, hip.F32, 16, 100, capacity=N)
        self.ref.upload_rows(X, 1)
        self.ref.upload_graph(*self.graph)
        self.ref.drop_walk_planes(refuse_for_good=True)
        if len(deleted):
            self.idx.Delete([int(d) for d in deleted])
            self.ref.Delete([int(d) for d in deleted])
        count, entry, max_level, levels, offs, nbrs = self.graph
        rows = np.zeros((count + 1, 768), dtype=np.float32)
        rows[1:] = X
        g = O.Graph(count, levels, max_level, entry, offs, nbrs, _bits(count, deleted))
        self.orc = O.OracleIndex.from_graph(768, O.COSINE, O.F32, 16, 100, rows, g)
        self.orc.set_arith(O.ARITH_HIP_WAVE)
        self._want = {}

    def want(self, ef, allow=None, key=None):
        """the oracle's answers to the distinct queries: computed once per (ef, allow list), shared, never modified"""
        if (ef, key) not in self._want:
            self._want[(ef, key)] = [self.orc.search(self.Q[b], K, allow=allow, ef=ef, counters=True) for b in range(NQ)]
        return self._want[(ef, key)]


@functools.lru_cache(maxsize=None)
def _plain():
    return Corpus(seed=11)


@functools.lru_cache(maxsize=None)
def _with_deleted():
    rng = np.random.default_rng(13)
    return Corpus(seed=12, deleted=tuple(rng.choice(np.arange(1, N + 1), N // 10, replace=False)))


def _check(c, ef, allow=None, key=None):
    import kektordb_amd as hip
    ra = c.idx.search_batch(c.Qt, K, ef, allow_bits=allow, trace=True, tie_flag=True)
    rb = c.ref.search_batch(c.Qt, K, ef, allow_bits=allow, trace=True, tie_flag=True)
    assert np.array_equal(ra[0], rb[0]), ef                                       # ids
    assert np.array_equal(ra[1].view(np.uint32), rb[1].view(np.uint32)), ef       # distance bits
    assert np.array_equal(ra[2], rb[2]), ef                                       # counts and tie flags
    assert np.array_equal(ra[3][0], rb[3][0]) and np.array_equal(ra[3][1], rb[3][1]), ef  # n_dist, n_hops
    ids, dist, cnt, (nd, nh) = ra
    tied = (cnt & hip.index.COUNT_TIED) != 0
    cnt = cnt & ~np.uint32(hip.index.COUNT_TIED)
    assert tied.sum() * 10 < tied.size, "a tenth of the walks tie: the oracle compares too little"
    want = c.want(ef, allow, key)
    for b in range(ids.shape[0]):
        if tied[b]:                      # (the reference's order of equal distances is its heaps': the dropped handle agreed above)
            continue
        oi, od, (ond, onh) = want[b % NQ]
        n = int(cnt[b])
        assert n == len(oi), (ef, b, n, len(oi))
        assert np.array_equal(ids[b, :n], oi), (ef, b, ids[b, :n], oi)
        assert np.array_equal(1.0 - dist[b, :n].astype(np.float64), od), (ef, b)
        assert (int(nd[b]), int(nh[b])) == (ond, onh), (ef, b, int(nd[b]), int(nh[b]), ond, onh)


@pytest.mark.parametrize("ef", EFS)
def test_twelve_walks_per_cu_same_answers(ef):
    _check(_plain(), ef)


@pytest.mark.parametrize("ef", EFS)
def test_twelve_walks_per_cu_deleted_nodes(ef):
    _check(_with_deleted(), ef)


@pytest.mark.parametrize("ef", EFS)
def test_twelve_walks_per_cu_allow_list_half(ef):
    rng = np.random.default_rng(50)
    allow = _bits(N, rng.choice(np.arange(1, N + 1), N // 2, replace=False))
    _check(_plain(), ef, allow=allow, key="half")


def _level0_new_neighbours(c, q, ef):
    """searchLayer on level 0 restated (float64 dots of the normalised rows): -> (new neighbours per hop, the k nearest ids)"""
    count, entry, max_level, levels, offs, nbrs = c.graph
    ep = entry
    for l in range(max_level, 0, -1):                                    # greedy descent: the oracle's own layers
        got, _ = c.orc.search_layer_raw(q, ep, 1, l, 1)
        ep = int(got[0])
    X = c.X.astype(np.float64)
    qd = q.astype(np.float64)
    d = lambda i: -float(X[i - 1] @ qd)
    visited = {ep}
    cand = [(d(ep), ep)]
    res = [(-cand[0][0], -ep)]                                           # max-heap on (distance, id)
    per_hop = []
    while cand:
        dc, cur = heapq.heappop(cand)
        if len(res) >= ef and dc > -res[0][0]:
            break
        fresh = [int(x) for x in nbrs[0][int(offs[0][cur]):int(offs[0][cur + 1])] if int(x) not in visited]
        visited.update(fresh)
        if fresh:
            per_hop.append(len(fresh))
        for x in fresh:
            dx = d(x)
            if len(res) < ef or dx < -res[0][0]:
                heapq.heappush(cand, (dx, x))
                heapq.heappush(res, (-dx, -x))
                if len(res) > ef:
                    heapq.heappop(res)
    top = sorted((-nd, -ni) for nd, ni in res)[:K]
    return per_hop, [i for _, i in top]


def test_corpus_produces_every_trip_shape():
    """CPU only in what it asserts: hops of the chosen corpus bring 1-4, 5-8, 9-16 and more than 16 new neighbours.  A restated walk
    counts only where it found the oracle's answer (float64 dots may order two near-equal candidates the other way)"""
    c = _plain()
    classes = {"1-4": 0, "5-8": 0, "9-16": 0, ">16": 0}
    agreed = 0
    for b in range(24):
        per_hop, top = _level0_new_neighbours(c, c.Q[b], 60)
        oi, _, _ = c.want(60)[b]
        if top != [int(x) for x in oi]:
            continue
        agreed += 1
        for n in per_hop:
            classes["1-4" if n <= 4 else "5-8" if n <= 8 else "9-16" if n <= 16 else ">16"] += 1
    assert agreed >= 12, agreed
    assert all(v > 0 for v in classes.values()), classes


def test_probe_gather_high_plane():
    """kdb_probe_gather(which = 2): KDB_ERR_UNSUPPORTED (-6) until a planes walk has made the planes, a positive rate after"""
    import kektordb_amd as hip
    c = _plain()
    idx = hip.HipIndex(768, hip.COSINE, hip.F32, 16, 100, capacity=N)
    idx.upload_rows(c.X, 1)
    idx.upload_graph(*c.graph)
    ms, nbytes = C.c_float(), C.c_uint64()
    assert idx.L.kdb_probe_gather(idx.h, 2, 100_000, C.byref(ms), C.byref(nbytes)) == -6
    with pytest.raises(hip.KdbError):
        idx.probe_gather(100_000, walk_hi=True)
    idx.search_batch(c.Qt, K, 60)                                        # 8400 queries: the planes kernel makes the planes
    rate = idx.probe_gather(100_000, walk_hi=True)
    assert rate > 0.0 and np.isfinite(rate)
    assert idx.L.kdb_probe_gather(idx.h, 2, 100_000, C.byref(ms), C.byref(nbytes)) == 0
    assert ms.value > 0.0 and nbytes.value > 0 and nbytes.value % 1536 == 0
    idx.close()
