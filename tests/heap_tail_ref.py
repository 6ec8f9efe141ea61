"""Corpora on which the reference's candidate heap grows long, and a restatement of its walk that measures how long.

searchLayerUnlocked pushes every accepted neighbour onto the candidate heap and pops one per hop; a neighbour is accepted while the
result set is not full or it beats the worst result; deleted nodes are pushed as candidates and never become results.  So the heap
is longest on an index in which almost every node is soft-deleted -- the reference's ordinary state between Delete and Vacuum:
the result set fills late or never and nearly every visited node is accepted.  With duplicate rows in it the walks also tie,
which is what sends a query to the heap-order walk (kektordb_amd/csrc/search_heap.hip), whose candidate heap keeps its first
entries in LDS and the rest in an HBM tail.

Shared by tests/test_oracle_peak.py (CPU: the oracle's peak counter against the restatement) and tests/test_gpu_heap_tail.py."""
import heapq

import numpy as np

L2, COSINE = 0, 1
F32, F16, I8 = 0, 1, 2
M, EFC = 16, 40
NQ = 24
DUP_GROUPS, DUP_SIZE = 6, 30


class TailCorpus:
    """rows, the oracle that built their graph (deleted nodes marked, ARITH_HIP_WAVE), the exported graph, the queries"""

    def __init__(self, O, n, dim, metric, prec, share, seed, dups=True):
        rng = np.random.default_rng(seed)
        X = rng.standard_normal((n, dim)).astype(np.float32)
        if prec == F16:
            X *= 0.25
        if dups:                                                         # six groups of 30 copies of one row
            for _ in range(DUP_GROUPS):
                X[rng.choice(n, DUP_SIZE, replace=False)] = X[int(rng.integers(0, n))]
        self.n, self.dim, self.metric, self.prec, self.share = n, dim, metric, prec, share
        orc = O.OracleIndex(dim, metric, prec, M, EFC, seed=4)
        if prec == I8:
            orc.set_absmax(float(np.quantile(np.abs(X / np.linalg.norm(X, axis=1, keepdims=True)), 0.999)))
        orc.add_many(X)
        levels = orc.export_graph().levels
        below = np.flatnonzero(np.asarray(levels[1:n + 1]) < orc.max_level) + 1   # (the descent still finds a live node on every layer)
        self.deleted = np.sort(rng.choice(below, int(share * below.size), replace=False))
        for d in self.deleted:
            orc.mark_deleted(int(d))
        self.graph = orc.export_graph()
        orc.set_arith(O.ARITH_HIP_WAVE)
        self.orc = orc
        self.X = X
        self.Q = (X[rng.integers(0, n, NQ)] + 0.01 * rng.standard_normal((NQ, dim))).astype(np.float32)
        self.dead = np.zeros(n + 1, dtype=bool)
        self.dead[self.deleted] = True
        self._want, self._dist = {}, None

    def want(self, k, ef):
        """the oracle's answers, counters and level-0 candidate-heap peaks of the queries: computed once, shared, never modified"""
        if (k, ef) not in self._want:
            out = []
            for b in range(self.Q.shape[0]):
                oi, od, ctr = self.orc.search(self.Q[b], k, ef=ef, counters=True)
                out.append((oi, od, ctr, self.orc.last_peak_candidates()))
            self._want[(k, ef)] = out
        return self._want[(k, ef)]

    def dist(self, b):
        """the oracle's own distance of query b to every row (index = id; row 0 unused)"""
        if self._dist is None:
            ids = np.arange(0, self.n + 1, dtype=np.uint32)
            ids[0] = 1
            self._dist = [self.orc.distances(self.Q[i], ids) for i in range(self.Q.shape[0])]
        return self._dist[b]


def restated_walk(c, b, k, ef):
    """searchLayerUnlocked restated with heapq over the exported graph on the oracle's distances of query b: every layer (ef 1 above
    level 0), deleted nodes candidates but never results -> (top-k ids, n_dist, n_hops, ids visited on level 0, the candidate
    heap's largest length on level 0); None where a layer ends without a result.  heapq orders equal distances by id, the reference
    by the history of its heaps: exact on rows without ties, an estimate (a few entries) on rows with duplicates."""
    g = c.graph
    d, dead = c.dist(b), c.dead
    ep, nd, nh = int(g.entry), 0, 0
    efq = max(ef, k)
    for l in range(int(g.max_level), -1, -1):
        ef_l = efq if l == 0 else 1
        off, nb = g.offsets[l], g.neighbors[l]
        visited = {ep}
        cand = [(d[ep], ep)]
        peak = 1
        res = [] if dead[ep] else [(-d[ep], -ep)]                       # max-heap on (distance, id)
        nd += 1
        while cand:
            dc, cur = heapq.heappop(cand)
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
                    peak = max(peak, len(cand))
                    if not dead[x]:
                        heapq.heappush(res, (-dx, -x))
                        if len(res) > ef_l:
                            heapq.heappop(res)
        if not res:
            return None
        top = sorted((-a, -i) for a, i in res)
        ep = top[0][1]
    return [i for _, i in top[:k]], nd, nh, len(visited), peak
