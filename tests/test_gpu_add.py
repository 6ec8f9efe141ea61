"""kdb_index_add = the reference's sequential Add (hnsw_index.go:472-809) on the device, one node after another, against the
restated Add (oracle orc_index_add) with forced levels: every list of every level in stored order, levels, entry point, maxLevel
and count.  The oracle computes in the GPU's accumulation order (ARITH_HIP_WAVE) from its first add; m = 8, efConstruction = 24,
so lists fill (mMax0 = 16) and prune within the first few dozen nodes.

int8 distances are exact, so every list must be identical.  float32 / float16 sum the pair distances inside selectNeighbors in
another order than the oracle: a list may differ where two such distances tie to rounding -- counted against the
project's bound for this one cause, max(2, lists / 500) (test_gpu_build.py, test_gpu_refine.py)."""
import ctypes as C

import numpy as np
import pytest

from conftest import make_corpus

pytestmark = pytest.mark.gpu

M, EFC = 8, 24
KDB_ERR_INVALID, KDB_ERR_UNSUPPORTED = -1, -6
STAT_SUMS = ("nodes_added", "forward_lists", "reverse_appended", "reverse_pruned", "tied_nodes", "reverse_skipped")


def draw_levels(n, seed, m=M):
    rng = np.random.default_rng(seed)
    return np.minimum(np.floor(-np.log(1.0 - rng.random(n)) / np.log(m)), 6).astype(np.int32)


def corpus(O, n, dim, prec, seed, law="uniform"):
    X = make_corpus(n, dim, law, seed=seed).astype(np.float32)
    if prec == O.F16:
        X = (X * 0.25).astype(np.float32)
    assert np.unique(X, axis=0).shape[0] == n, "duplicate rows"
    return X


def new_pair(O, hip, X, metric, prec, m=M, efc=EFC):
    n, dim = X.shape
    orc = O.OracleIndex(dim, metric, prec, m, efc, seed=5)
    orc.set_arith(O.ARITH_HIP_WAVE)
    idx = hip.HipIndex(dim, metric, prec, m, efc, capacity=n + 8)
    if prec == O.I8:
        orc.set_absmax(float(np.abs(X).max()))
        idx.set_quantizer(orc.absmax)
    return orc, idx


def oracle_add(orc, X, levels, lo, hi):
    """ids lo..hi (1-based, inclusive) into the oracle"""
    for i in range(lo, hi + 1):
        assert orc.add(X[i - 1], level=int(levels[i - 1])) == i


def gpu_add(idx, orc, O, prec, levels, lo, hi, efc=EFC):
    """the stored form of ids lo..hi goes up, then ONE kdb_index_add call"""
    idx.upload_rows(orc.rows()[lo:hi + 1], lo)
    if prec == O.I8:
        idx.upload_norms(orc.norms()[lo:hi + 1], lo)
    return idx.add(lo, levels[lo - 1:hi], efc)


def dense(cnt, max_level, offs, nbrs, rows=None, m=M):
    """per level a [rows, 2m] matrix of the lists in stored order, 0-filled"""
    rows = cnt + 1 if rows is None else rows
    out = []
    for l in range(max_level + 1):
        off = np.asarray(offs[l][:cnt + 2], dtype=np.int64)
        lens = np.diff(off)
        assert lens.max(initial=0) <= (2 * m if l == 0 else m), (l, int(lens.max()))
        tot = int(off[cnt + 1])
        mat = np.zeros((rows, 2 * m), dtype=np.uint32)
        mat[np.repeat(np.arange(cnt + 1), lens), np.arange(tot) - np.repeat(off[:cnt + 1], lens)] = np.asarray(nbrs[l][:tot])
        out.append(mat)
    return out


def gpu_dense(idx, rows=None, m=M):
    cnt, entry, mlv, glv, offs, nbrs = idx.download_graph()
    return (cnt, entry, mlv, glv[:cnt + 1].copy()), dense(cnt, mlv, offs, nbrs, rows, m)


def orc_dense(orc, rows=None, m=M):
    og = orc.export_graph()
    return og, (og.count, og.entry, og.max_level, og.levels[:og.count + 1].copy()), dense(og.count, og.max_level, og.offsets, og.neighbors, rows, m)


def lists_differing(a, b):
    """number of (node, level) lists that differ between two dense graphs (the shorter one padded with empty lists)"""
    bad = 0
    for l in range(max(len(a), len(b))):
        x = a[l] if l < len(a) else np.zeros_like(b[l])
        y = b[l] if l < len(b) else np.zeros_like(a[l])
        r = max(x.shape[0], y.shape[0])
        x = np.pad(x, ((0, r - x.shape[0]), (0, 0)))
        y = np.pad(y, ((0, r - y.shape[0]), (0, 0)))
        bad += int(np.count_nonzero(np.any(x != y, axis=1)))
    return bad


def assert_same_header(gh, oh):
    assert gh[:3] == oh[:3], (gh[:3], oh[:3])
    assert np.array_equal(gh[3][1:], oh[3][1:])


def assert_list_invariants(gd, cnt, glv, m=M):
    """a dense graph of cnt nodes: lists within their width, no id beyond cnt, no own node, no hole, no node twice, nothing above
    a node's level"""
    for l, mat in enumerate(gd):
        width = 2 * m if l == 0 else m
        assert not mat[:, width:].any()
        assert mat.max() <= cnt
        own = np.arange(cnt + 1, dtype=np.uint32)[:, None]
        assert not np.any((mat == own) & (mat != 0)), "a list names its own node"
        assert not mat[0].any()
        lens = np.count_nonzero(mat, axis=1)
        assert np.all((np.arange(2 * m)[None, :] < lens[:, None]) == (mat != 0)), "a hole inside a list"
        s = np.sort(mat, axis=1)
        assert not np.any((s[:, 1:] == s[:, :-1]) & (s[:, 1:] != 0)), "a list names a node twice"
        assert not mat[glv < l].any()


CALLS_EXACT = (1, 1, 1, 5, 17, 64, 300)


@pytest.fixture(scope="module")
def int8_from_empty(oracle, hip):
    """test 1's inserts, kept for test 7: int8 cosine, n = 1500, dim 64, from an index without a graph, many nodes per call"""
    O = oracle
    n, dim = 1500, 64
    X = corpus(O, n, dim, O.I8, 11)
    levels = draw_levels(n, 12)
    levels[[0, 3, 40, 200]] = (0, 4, 6, 6)          # asks far above the top: capped to 1, 2, 3 -- each raises maxLevel
    orc, idx = new_pair(O, hip, X, O.COSINE, O.I8)
    sizes = list(CALLS_EXACT) + [n - sum(CALLS_EXACT)]
    pos, raised, stats, per_call = 0, 0, {k: 0 for k in STAT_SUMS}, []
    for sz in sizes:
        lo, hi = pos + 1, pos + sz
        for i in range(lo, hi + 1):
            before = orc.max_level
            oracle_add(orc, X, levels, i, i)
            raised += int(before >= 0 and orc.max_level > before)
        st = gpu_add(idx, orc, O, O.I8, levels, lo, hi)
        for k in STAT_SUMS:
            stats[k] += st[k]
        gh, gd = gpu_dense(idx)
        og, oh, od = orc_dense(orc)
        per_call.append((sz, gh, oh, lists_differing(gd, od), (st["entry"], st["max_level"])))
        pos = hi
    return dict(O=O, orc=orc, idx=idx, X=X, n=n, dim=dim, raised=raised, stats=stats, per_call=per_call)


def test_add_int8_exact_from_empty(int8_from_empty):
    """1. int8 cosine from an empty index, calls of 1, 1, 1, 5, 17, 64, 300 and the rest: after every call every list is the oracle's"""
    r = int8_from_empty
    assert r["raised"] >= 3, r["raised"]
    for sz, gh, oh, bad, (entry, max_level) in r["per_call"]:
        assert_same_header(gh, oh)
        assert (entry, max_level) == oh[1:3]
        assert bad == 0, (sz, bad)
    st = r["stats"]
    print("int8 from empty:", st)
    assert st["nodes_added"] == r["n"] and st["forward_lists"] >= r["n"] - 1
    assert st["tied_nodes"] == 0 and st["reverse_skipped"] == 0 and st["reverse_pruned"] > 0 and st["reverse_appended"] > 0


@pytest.mark.parametrize("metric,prec,dim,seeded", [("L2", "F32", 48, False), ("COSINE", "F32", 100, True), ("L2", "F16", 64, False)])
def test_add_float_per_node(oracle, hip, metric, prec, dim, seeded):
    """2. float32 L2 / float32 cosine / float16 L2, n = 400, one node per call, compared after every call; `seeded`: the first 50
    nodes are the oracle's, uploaded as a graph -- the other cases start from an index without one"""
    O = oracle
    metric, prec = getattr(O, metric), getattr(O, prec)
    n = 400
    X = corpus(O, n, dim, prec, 21 + dim)
    levels = draw_levels(n, 22 + dim)
    orc, idx = new_pair(O, hip, X, metric, prec)
    start = 1
    if seeded:
        oracle_add(orc, X, levels, 1, 50)
        idx.upload_rows(orc.rows()[1:51], 1)
        idx.upload_graph_obj(orc.export_graph())
        start = 51
    bad = total = tied = 0
    _, _, prev = orc_dense(orc, n + 1)
    for i in range(start, n + 1):
        oracle_add(orc, X, levels, i, i)
        st = gpu_add(idx, orc, O, prec, levels, i, i)
        tied += st["tied_nodes"]
        og, oh, od = orc_dense(orc, n + 1)
        total += lists_differing(prev, od)                   # the lists the oracle's own add changed
        prev = od
        gh, gd = gpu_dense(idx, n + 1)
        assert_same_header(gh, oh)
        assert (st["entry"], st["max_level"]) == oh[1:3]
        d = lists_differing(gd, od)
        if d:                                                # a rounding tie: the next node starts from equal graphs again
            bad += d
            idx.upload_graph_obj(og)
    print(f"add metric {metric} prec {prec} seeded {seeded}: {total} lists changed by the oracle's adds, {bad} differed (rounding ties)")
    assert total > 4 * n
    assert tied == 0
    assert bad <= max(2, total // 500), (bad, total)


def test_add_one_call_equals_many(oracle, hip):
    """3. GPU against GPU: 600 nodes in one call and in 600 calls of one give bit-identical graphs and equal summed statistics"""
    O = oracle
    n, dim = 600, 100
    X = corpus(O, n, dim, O.F32, 31)
    levels = draw_levels(n, 32)
    rows = X / np.linalg.norm(X, axis=1, keepdims=True).astype(np.float32)
    a = hip.HipIndex(dim, O.COSINE, O.F32, M, EFC, capacity=n + 8)
    b = hip.HipIndex(dim, O.COSINE, O.F32, M, EFC, capacity=n + 8)
    a.upload_rows(rows, 1)
    b.upload_rows(rows, 1)
    sa = a.add(1, levels, EFC)
    sb = {k: 0 for k in STAT_SUMS}
    for i in range(1, n + 1):
        s1 = b.add(i, levels[i - 1:i], EFC)
        for k in STAT_SUMS:
            sb[k] += s1[k]
    assert {k: sa[k] for k in STAT_SUMS} == sb
    assert (sa["entry"], sa["max_level"]) == (s1["entry"], s1["max_level"])
    ga, gb = a.download_graph(), b.download_graph()
    assert ga[:3] == gb[:3] and ga[0] == n and ga[2] >= 1
    assert np.array_equal(ga[3], gb[3])
    for l in range(ga[2] + 1):
        assert np.array_equal(ga[4][l], gb[4][l]) and np.array_equal(ga[5][l], gb[5][l]), l
    assert sa["nodes_added"] == n and sa["reverse_pruned"] > 0


def test_add_with_deleted_nodes(oracle, hip):
    """4. int8, n = 800: after 500 nodes 60 are deleted (the entry point among them), then the rest is added: identical lists, no
    new list names a deleted id, and full neighbour lists that are pruned drop their links to deleted nodes (:756-761)"""
    O = oracle
    n, dim, n0 = 800, 64, 500
    X = corpus(O, n, dim, O.I8, 41)
    levels = draw_levels(n, 42)
    orc, idx = new_pair(O, hip, X, O.COSINE, O.I8)
    oracle_add(orc, X, levels, 1, n0)
    gpu_add(idx, orc, O, O.I8, levels, 1, n0)
    rng = np.random.default_rng(43)
    dead = set(int(x) for x in rng.choice(np.arange(1, n0 + 1), 60, replace=False))
    if orc.entry not in dead:
        dead.discard(next(iter(dead)))
        dead.add(orc.entry)
    dead = np.array(sorted(dead), dtype=np.uint32)
    assert dead.size == 60 and orc.entry in dead
    for d in dead:
        orc.mark_deleted(int(d))
    idx.Delete(dead)
    _, links_before, n_dead = idx.dead_link_scan()
    assert n_dead == 60 and links_before > 0
    _, before = gpu_dense(idx, n + 1)
    pos, stats = n0, {k: 0 for k in STAT_SUMS}
    for sz in (1, 50, n - n0 - 51):
        oracle_add(orc, X, levels, pos + 1, pos + sz)
        st = gpu_add(idx, orc, O, O.I8, levels, pos + 1, pos + sz)
        for k in STAT_SUMS:
            stats[k] += st[k]
        gh, gd = gpu_dense(idx, n + 1)
        og, oh, od = orc_dense(orc, n + 1)
        assert_same_header(gh, oh)
        assert lists_differing(gd, od) == 0
        pos += sz
    assert stats["tied_nodes"] == 0 and stats["reverse_skipped"] == 0 and stats["reverse_pruned"] > 0
    is_dead = np.zeros(n + 2, dtype=bool)
    is_dead[dead] = True
    dropped = 0
    for l, m in enumerate(gd):
        assert not is_dead[m[n0 + 1:]].any(), "a new node's list names a deleted id"
        if l < len(before):
            full = np.count_nonzero(before[l], axis=1) == (2 * M if l == 0 else M)
            changed = np.any(before[l] != m, axis=1)
            live = ~is_dead[:n + 1]
            pruned = full & changed & live
            assert not is_dead[m[pruned]].any(), "a pruned list kept a link to a deleted node"
            dropped += int(np.count_nonzero(is_dead[before[l][pruned]]))
    _, links_after, n_dead = idx.dead_link_scan()
    assert n_dead == 60
    # (lists that filled up after the deletions and were pruned then dropped theirs too: at least `dropped` are gone, none came)
    assert dropped > 0 and links_after <= links_before - dropped, (links_before, links_after, dropped)
    assert links_after == sum(int(np.count_nonzero(is_dead[m[~is_dead[:n + 1]]])) for m in gd)


def test_add_ties_are_reported(oracle, hip):
    """5. float32 L2 with 20 duplicated rows: walks hold two nodes at equal distance -- reported in tied_nodes, and the graph keeps
    its invariants; no list-for-list claim.  The corpus is clustered: with m = 8, efConstruction = 24 the REFERENCE's own graph
    (the oracle's, same rows and levels) leaves 2 to 5 of 300 nodes unreachable at ef = 24 on 48-d uniform or normal rows and none
    on clustered ones -- checked here as a control, so that a miss on the device side is the device's."""
    O = oracle
    n, dim = 300, 48
    X = corpus(O, n, dim, O.F32, 51, law="clustered")
    X[100:120] = X[0:20]
    levels = draw_levels(n, 52)
    orc = O.OracleIndex(dim, O.L2, O.F32, M, EFC, seed=5)
    orc.set_arith(O.ARITH_HIP_WAVE)
    oracle_add(orc, X, levels, 1, n)
    for i in range(n):
        oi, od = orc.search(X[i], 1, ef=EFC)
        assert len(oi) == 1 and od[0] == 0, ("control: the reference's own graph does not reach node", i + 1)
    idx = hip.HipIndex(dim, O.L2, O.F32, M, EFC, capacity=n + 8)
    idx.upload_rows(X, 1)
    st = idx.add(1, levels, EFC)
    assert st["nodes_added"] == n and st["tied_nodes"] > 0
    (cnt, entry, mlv, glv), gd = gpu_dense(idx)
    assert cnt == n and 1 <= entry <= n
    assert_list_invariants(gd, cnt, glv)
    ids, dist, c = idx.search_batch(X, 1, EFC)
    twin = np.arange(1, n + 1)
    twin[0:20], twin[100:120] = np.arange(101, 121), np.arange(1, 21)
    assert np.all(c == 1) and np.all(dist[:, 0] == 0)
    assert np.all((ids[:, 0] == np.arange(1, n + 1)) | (ids[:, 0] == twin))


def test_add_arguments(oracle, hip):
    """6. refusals leave count, graph and entry as they were; a correct call afterwards still matches the oracle"""
    O = oracle
    from kektordb_amd import _lib
    n, dim = 120, 64
    X = corpus(O, n, dim, O.I8, 61)
    levels = draw_levels(n, 62)
    orc, idx = new_pair(O, hip, X, O.COSINE, O.I8)
    oracle_add(orc, X, levels, 1, 80)
    gpu_add(idx, orc, O, O.I8, levels, 1, 80)
    oracle_add(orc, X, levels, 81, n)
    idx.upload_rows(orc.rows()[81:n + 1], 81)
    idx.upload_norms(orc.norms()[81:n + 1], 81)
    before = idx.download_graph()
    lv = np.ascontiguousarray(levels[80:], dtype=np.uint8)
    L, st = idx.L, _lib.AddStats()

    def call(first, cnt, lvp, efc=EFC):
        return L.kdb_index_add(idx.h, first, cnt, lvp, C.byref(_lib.AddParams(efc, 0)), C.byref(st))

    lvp = lv.ctypes.data_as(C.c_void_p)
    assert call(80, 5, lvp) == KDB_ERR_INVALID                # first_id != count + 1 (the slot re-use is add_batch's alone)
    assert call(82, 5, lvp) == KDB_ERR_INVALID
    assert call(81, n + 8 - 80 + 1, lvp) == KDB_ERR_INVALID   # beyond capacity
    assert call(81, 5, None) == KDB_ERR_INVALID               # NULL levels
    assert call(81, 5, lvp, 513) == KDB_ERR_UNSUPPORTED
    assert call(81, 0, lvp) == 0 and call(81, 0, None) == 0
    after = idx.download_graph()
    assert before[:3] == after[:3] == (80, before[1], before[2])
    assert np.array_equal(before[3], after[3])
    for l in range(before[2] + 1):
        assert np.array_equal(before[4][l], after[4][l]) and np.array_equal(before[5][l], after[5][l])
    assert L.kdb_index_add(idx.h, 81, lv.size, lvp, None, None) == 0     # params and stats may be NULL: the index's efConstruction
    gh, gd = gpu_dense(idx)
    og, oh, od = orc_dense(orc)
    assert_same_header(gh, oh)
    assert lists_differing(gd, od) == 0


def test_added_graph_is_searchable(int8_from_empty):
    """7. after test 1's inserts the ordinary search path answers as the oracle does on its own graph, ids and distances bit for bit
    (stale derived state -- the upper-slot table, ranking copies -- would show here)"""
    r = int8_from_empty
    orc, idx = r["orc"], r["idx"]
    Q = make_corpus(200, r["dim"], "uniform", seed=71)
    k, ef = 10, 50
    ids, dist, cnt = idx.search_batch(Q, k, ef, dist64=True, heap_order=True)
    for b in range(Q.shape[0]):
        oi, od = orc.search(Q[b], k, ef=ef)
        c = int(cnt[b])
        assert c == len(oi) == k
        assert np.array_equal(ids[b, :c], oi) and np.array_equal(dist[b, :c], od), b
