"""The rare paths of the planes walk's hop loop under the three-wave kernel: VisHash::migrate with the bitset branch of
test_and_set behind it, the pending list of traversal-only candidates (deleted nodes), the tie bookkeeping.  The hop loop of
hnsw_search_kernel<f32, cosine, 768 columns, one-slot beam, planes> keeps none of their values in registers or scratch across a hop
any more (they are made again inside the rare path, kdb_lane_again), so these paths are pinned here: 6000 rows of which SHARE of
the nodes below the graph's top level are deleted (the descent still finds a live node on every layer), ef 24, 60 and 64 (the
one-slot beam), 8400 queries (300 distinct ones, tiled: the one-wave kernel, LDS reused by a second walk).  Every comparison is exact -- ids in order, distance bits,
counts, the tie bit, per-query n_dist and n_hops -- against a handle whose planes were dropped for good and against the oracle's
walk; the launch-shape probe says that the planes kernel ran on the one handle and the float32-row kernel on the other.

That the corpus takes the paths is asserted on the CPU before any comparison, from a restatement of the walk on the oracle's own
distances that must reproduce the oracle's answer and counters query for query:
  * at least 32 of the 300 queries visit more ids on level 0 than the limit of the 2048-entry hash the launch uses
    (VisHash::begin_layer: 2048 - 256 - 64 = 1728): their visited sets migrate to the bitset in the middle of the walk;
  * no query ever has more deleted candidates pending than the list holds (kdb_nr_cap: 2048 entries at this many deleted nodes):
    nothing is dropped, the walk stays the reference's.
None of the existing planes tests reaches the first condition (their walks visit a few hundred ids)."""
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
SHARE = 0.96        # of the nodes below the top level, deleted.  Settled with the oracle alone on a graph the oracle built from the same
                    # rows: 0.95 / 0.96 / 0.965 gave 73 / 183 / 227 queries over the limit at ef 24 (all 300 at ef 60 and 64) and at most
                    # 1430 / 1608 / 1836 candidates pending at ef 64; random deletion of 0.93 of ALL rows gave 4 at ef 24, 0.95 no live
                    # node on the top layer
HASH_LIMIT = 2048 - 256 - 64
NR_CAP = 2048       # kdb_nr_cap(n_deleted >= 2047)


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

    def __init__(self, X, Q, deleted=()):
        import kektordb_amd as hip
        from oracle import oracle as O
        O.build()
        n = X.shape[0]
        self.X, self.Q = X, Q
        self.Qt = np.tile(Q, (REPS, 1))
        self.idx = hip.HipIndex(768, hip.COSINE, hip.F32, 16, 100, capacity=n)
        self.idx.upload_rows(X, 1)
        self.idx.build(n, batch=512, ef_construction=100, seed=3)
        self.graph = self.idx.download_graph()
        if callable(deleted):                                            # (chosen from the graph: its levels)
            deleted = deleted(self.graph)
        self.deleted = np.asarray(sorted(int(d) for d in deleted), dtype=np.int64)
        self.ref = hip.HipIndex(768, hip.COSINE, hip.F32, 16, 100, capacity=n)
        self.ref.upload_rows(X, 1)
        self.ref.upload_graph(*self.graph)
        self.ref.drop_walk_planes(refuse_for_good=True)
        if self.deleted.size:
            self.idx.Delete([int(d) for d in self.deleted])
            self.ref.Delete([int(d) for d in self.deleted])
        count, entry, max_level, levels, offs, nbrs = self.graph
        rows = np.zeros((count + 1, 768), dtype=np.float32)
        rows[1:] = X
        g = O.Graph(count, levels, max_level, entry, offs, nbrs, _bits(count, self.deleted))
        self.orc = O.OracleIndex.from_graph(768, O.COSINE, O.F32, 16, 100, rows, g)
        self.orc.set_arith(O.ARITH_HIP_WAVE)
        self.dead = np.zeros(count + 1, dtype=bool)
        self.dead[self.deleted] = True
        self._want, self._dist = {}, None

    def want(self, ef):
        """the oracle's answers to the distinct queries: computed once per ef, shared, never modified"""
        if ef not in self._want:
            self._want[ef] = [self.orc.search(self.Q[b], K, ef=ef, counters=True) for b in range(self.Q.shape[0])]
        return self._want[ef]

    def dist(self, b):
        """the oracle's own distance of query b to every row (index = id; row 0 unused)"""
        if self._dist is None:
            ids = np.arange(0, self.X.shape[0] + 1, dtype=np.uint32)
            ids[0] = 1
            self._dist = [self.orc.distances(self.Q[i], ids) for i in range(self.Q.shape[0])]
        return self._dist[b]


def restated_walk(c, b, ef):
    """searchLayerUnlocked restated over the downloaded graph on the oracle's distances of query b: every layer (ef 1 above level 0),
    deleted nodes candidates but never results -> (top-K ids, n_dist, n_hops, ids visited on level 0, most deleted candidates pending
    at once on level 0); None where a layer ends without a result"""
    count, entry, max_level, levels, offs, nbrs = c.graph
    d, dead = c.dist(b), c.dead
    ep, nd, nh = int(entry), 0, 0
    for l in range(int(max_level), -1, -1):
        ef_l = ef if l == 0 else 1
        off, nb = offs[l], nbrs[l]
        visited = {ep}
        cand = [(d[ep], ep)]
        res = [] if dead[ep] else [(-d[ep], -ep)]                       # max-heap on (distance, id)
        pend = most = 1 if dead[ep] else 0
        nd += 1
        while cand:
            dc, cur = heapq.heappop(cand)
            if dead[cur]:
                pend -= 1
            if len(res) >= ef_l and dc > -res[0][0]:
                break
            nh += 1
            fresh = [int(x) for x in nb[int(off[cur]):int(off[cur + 1])] if int(x) not in visited]
            visited.update(fresh)
            nd += len(fresh)
            for x in fresh:
                dx = d[x]
                if len(res) < ef_l or dx < -res[0][0]:
                    heapq.heappush(cand, (dx, x))
                    if dead[x]:
                        pend += 1
                        most = max(most, pend)
                    else:
                        heapq.heappush(res, (-dx, -x))
                        if len(res) > ef_l:
                            heapq.heappop(res)
        if not res:
            return None
        top = sorted((-a, -i) for a, i in res)
        ep = top[0][1]
    return [i for _, i in top[:K]], nd, nh, len(visited), most


def path_census(c, ef):
    """-> (queries whose restated walk is the oracle's, of those: how many outgrow the hash on level 0, the most deleted candidates any
    of them had pending at once, the queries that could not be restated)"""
    agreed = over = most = 0
    missed = []
    for b in range(c.Q.shape[0]):
        oi, _, (ond, onh) = c.want(ef)[b]
        r = restated_walk(c, b, ef)
        if r is None or r[0] != [int(x) for x in oi] or (r[1], r[2]) != (ond, onh):
            missed.append(b)
            continue
        agreed += 1
        over += r[3] > HASH_LIMIT
        most = max(most, r[4])
    return agreed, over, most, missed


def assert_paths_taken(c, ef):
    agreed, over, most, missed = path_census(c, ef)
    # (a walk the restatement cannot follow -- equal distances popped in another order -- proves nothing about its pending list: none allowed)
    assert not missed, (ef, missed[:10])
    assert over >= 32, (ef, over)
    assert most <= NR_CAP - 1, (ef, most)
    assert c.deleted.size >= 2047                                        # (the list has its largest capacity: NR_CAP)


@functools.lru_cache(maxsize=None)
def _mostly_deleted():
    X = _clustered(N, 768, seed=61)

    def below_the_top(graph):
        count, _, max_level, levels = graph[:4]
        base = np.flatnonzero(np.asarray(levels[1:count + 1]) < max_level) + 1
        return np.random.default_rng(63).choice(base, int(SHARE * base.size), replace=False)

    return Corpus(X, _queries(X, NQ, seed=62), deleted=below_the_top)


def check(c, ef, oracle=True, **flags):
    import kektordb_amd as hip
    ra = c.idx.search_batch(c.Qt, K, ef, trace=True, tie_flag=True, **flags)
    sa = c.idx.launch_shape()[0]
    rb = c.ref.search_batch(c.Qt, K, ef, trace=True, tie_flag=True, **flags)
    sb = c.ref.launch_shape()[0]
    # the kernel under test really ran: one wave per query, 768 columns, one-slot beam, LDS hash, rows from the walk planes -- and the
    # other handle walked the float32 rows (were the planes refused, both would run one kernel and agree about nothing)
    if not flags.get("heap_order"):      # (with the heap-order pass the same handles were checked by the call before, without it)
        assert (sa["search"], sa["nch"], sa["bs"], sa["waves"], sa["planes"], sa["vis_hash_words"]) == (1, 12, 1, 1, 1, 2048), sa
        assert (sb["search"], sb["nch"], sb["bs"], sb["waves"], sb["planes"]) == (1, 12, 1, 1, 0), sb
    assert np.array_equal(ra[0], rb[0]), ef                                       # ids
    assert np.array_equal(ra[1].view(np.uint32), rb[1].view(np.uint32)), ef       # distance bits
    assert np.array_equal(ra[2], rb[2]), ef                                       # counts and tie flags
    assert np.array_equal(ra[3][0], rb[3][0]) and np.array_equal(ra[3][1], rb[3][1]), ef  # n_dist, n_hops
    ids, dist, cnt, (nd, nh) = ra
    tied = (cnt & hip.index.COUNT_TIED) != 0
    cnt = cnt & ~np.uint32(hip.index.COUNT_TIED)
    if not oracle:
        return tied
    if flags.get("heap_order"):
        assert not tied.any()                                            # heap order resolves every tie
    assert tied.sum() * 10 < tied.size, "a tenth of the walks tie: the oracle compares too little"
    want = c.want(ef)
    nq = c.Q.shape[0]
    for b in range(ids.shape[0]):
        if tied[b]:                      # (the reference's order of equal distances is its heaps': the dropped handle agreed above)
            continue
        oi, od, (ond, onh) = want[b % nq]
        n = int(cnt[b])
        assert n == len(oi), (ef, b, n, len(oi))
        assert np.array_equal(ids[b, :n], oi), (ef, b, ids[b, :n], oi)
        assert np.array_equal(1.0 - dist[b, :n].astype(np.float64), od), (ef, b)
        assert (int(nd[b]), int(nh[b])) == (ond, onh), (ef, b, int(nd[b]), int(nh[b]), ond, onh)
    return tied


@pytest.mark.parametrize("ef", EFS)
def test_visited_set_outgrows_the_hash_pending_list_never_drops(ef):
    c = _mostly_deleted()
    assert_paths_taken(c, ef)                                            # CPU: the corpus takes the paths
    check(c, ef)
    ctr = c.idx.counters()
    assert ctr["n_dropped"] == 0, ctr


# ---- ties ------------------------------------------------------------------------------------------------------------------------------
DUP_STRIDE = 256    # one row in 256 is an exact copy of its predecessor: a quarter to a third of the walks meet a pair


@functools.lru_cache(maxsize=None)
def _duplicates(stride=DUP_STRIDE):
    """exact copies among the rows: equal distances wherever a walk meets a pair"""
    X = _clustered(N, 768, seed=71)
    X[stride - 1::stride] = X[stride - 2::stride]
    return Corpus(X, _queries(X, NQ, seed=72))


@pytest.mark.parametrize("ef", EFS)
def test_tie_and_heap_order_flags_on_duplicate_rows(ef):
    """as test_gpu_walk_planes.py::test_parity_tie_and_heap_order_flags, on rows that do tie: with the tie flag alone the walks that
    report a tie are compared with the dropped handle only, under KDB_SEARCH_HEAP_ORDER every walk is the oracle's"""
    c = _duplicates()
    tied = check(c, ef, oracle=False)
    assert tied.any(), "no walk ties: the case does not reach the tie bookkeeping"
    check_tied_skipped(c, ef)
    check(c, ef, heap_order=True)


def check_tied_skipped(c, ef):
    import kektordb_amd as hip
    ids, dist, cnt, (nd, nh) = c.idx.search_batch(c.Qt, K, ef, trace=True, tie_flag=True)
    tied = (cnt & hip.index.COUNT_TIED) != 0
    assert tied.sum() < tied.size, "every query ties: the case compares nothing"
    cnt = cnt & ~np.uint32(hip.index.COUNT_TIED)
    want = c.want(ef)
    for b in np.flatnonzero(~tied):
        oi, od, (ond, onh) = want[b % c.Q.shape[0]]
        n = int(cnt[b])
        assert n == len(oi) and np.array_equal(ids[b, :n], oi), (ef, b)
        assert np.array_equal(1.0 - dist[b, :n].astype(np.float64), od), (ef, b)
        assert (int(nd[b]), int(nh[b])) == (ond, onh), (ef, b)
