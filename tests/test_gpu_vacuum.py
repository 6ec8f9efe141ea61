"""kdb_index_vacuum / kdb_index_dead_link_scan = GraphOptimizer.Vacuum (pkg/core/hnsw/optimizer.go:133-277) on the device.

EXPECTED STATE after a vacuum, computed here in numpy from the start graph (`case.lists`, `case.deleted` of test_gpu_refine.Case):
  D = the deleted ids;  R = every live node with at least one dead link (an entry that names an id of D or no node) on any of
  its levels, ascending;  the lists of R are `case.restate(R)` (Refine over R on the SNAPSHOT: the reference's one-by-one repair
  order is not mirrored);  the lists of D are empty;  every other list is word for word as before;  a live entry point stays, a
  deleted one is replaced by the lowest live id with max_level = that node's level (the reference's rule, :232-250), or with
  KDB_VACUUM_ELECT_TOP_LEVEL by the live node of the highest level (lowest id among equals);  no live node: entry 0, max_level -1;
  levels and deleted bits are unchanged, the rows of D are zero, live rows are untouched.
Tolerance (test_gpu_refine.check_refined's): int8 lists identical without exception; float32 / float16 may differ in at most
max(2, lists // 500) REPAIRED lists per case (rounding ties inside selectNeighbors); everything else is exact.

download_graph hands out the levels 0..max_level only, and the reference rule usually leaves max_level 0: to look at the upper
lists the tests raise the header through kdb_index_set_entry for the download and put it back."""
import functools

import numpy as np
import pytest

from test_gpu_refine import COSINE, F32, I8, L2, Case, _case, downloaded_lists

ELECT_TOP = dict(elect_top_level=True)


# ---- start graphs --------------------------------------------------------------------------------------------------------------
def _with_dead(case, dead):
    """a Case whose deleted ids are exactly `dead` (Case itself only draws them at random)"""
    assert not case.deleted.any()
    for d in dead:
        case.orc.mark_deleted(int(d))
    case.g = case.orc.export_graph()
    db = case.g.deleted_bits
    case.deleted = np.array([(int(db[i >> 6]) >> (i & 63)) & 1 for i in range(case.count + 1)], dtype=bool)
    assert sorted(np.nonzero(case.deleted)[0].tolist()) == sorted({int(d) for d in dead})
    case._restated = {}
    return case


@functools.lru_cache(maxsize=None)
def _vcase(name):
    from oracle import oracle as O
    O.build()
    if name == "few":
        return Case(O, COSINE, F32, 3000, 96, 16, 60, seed=21, deleted_frac=0.01, delete_entry=True)
    if name == "levels5":
        return Case(O, L2, F32, 1500, 64, 4, 8, seed=13, level_cap=4, deleted_frac=0.05, delete_entry=True)
    if name == "first3":                                        # ids 1..3 and the entry point deleted: the lowest live id is 4
        c = Case(O, COSINE, F32, 200, 96, 16, 60, seed=22)
        assert c.g.entry > 4
        return _with_dead(c, [1, 2, 3, c.g.entry])
    if name == "alldead":                                       # the 40-node "tiny" shape, every id marked
        c = Case(O, COSINE, F32, 40, 96, 16, 60, seed=14)
        return _with_dead(c, range(1, c.count + 1))
    return _case(name)                                          # "deleted", "f16", "i8", "cos": test_gpu_refine's own


def is_dead_link(case, nb):
    return not (1 <= nb <= case.count) or bool(case.deleted[nb])


@functools.lru_cache(maxsize=None)
def expected(name):
    """-> (case, D, R, dead links in live nodes' lists, {(node, level): new list} for R)"""
    case = _vcase(name)
    D = [x for x in range(1, case.count + 1) if case.deleted[x]]
    R, links = [], 0
    for x in range(1, case.count + 1):
        if case.deleted[x]:
            continue
        n = sum(1 for lst in case.lists[x] for nb in lst if is_dead_link(case, nb))
        links += n
        if n:
            R.append(x)
    if not R:
        return case, D, R, links, {}
    if case.prec != F32 or len(R) == case.count - len(D):       # the Python layer search is slow: share test_gpu_refine's full restatement
        full, _ = case.restate()                                # (same snapshot: a subset gives the same lists)
        rs = set(R)
        new = {k: v for k, v in full.items() if k[0] in rs}
    else:
        new, _ = case.restate(R)
    return case, D, R, links, new


def elected(case, top_level):
    """step 4 -> (entry, max_level, changed)"""
    if not case.deleted[case.g.entry]:
        return case.g.entry, case.g.max_level, 0
    live = [x for x in range(1, case.count + 1) if not case.deleted[x]]
    if not live:
        return 0, -1, 1
    if not top_level:
        return live[0], int(case.g.levels[live[0]]), 1
    top = max(int(case.g.levels[x]) for x in live)
    return min(x for x in live if int(case.g.levels[x]) == top), top, 1


def all_lists(case, idx):
    """-> ((count, entry, max_level, levels), lists [node][level]) with every level a live node has: the header is raised for the
    download where the vacuum lowered max_level, and put back"""
    cnt, entry, mlv = idx.graph_info()
    live = [x for x in range(1, case.count + 1) if not case.deleted[x]]
    top = max((int(case.g.levels[x]) for x in live), default=-1)
    if mlv < top:
        idx.set_entry(min(x for x in live if int(case.g.levels[x]) == top), top)
    if idx.graph_info()[2] < 0:
        return (cnt, entry, mlv, None), None
    cnt2, _, vis, levels, offs, nbrs = idx.download_graph()
    out = [[] for _ in range(cnt2 + 1)]
    for x in range(1, cnt2 + 1):
        for l in range(min(int(levels[x]), vis) + 1):
            out[x].append(nbrs[l][int(offs[l][x]):int(offs[l][x + 1])].tolist())
    if mlv < top:
        idx.set_entry(entry, mlv)
    assert idx.graph_info() == (cnt, entry, mlv)
    return (cnt, entry, mlv, levels), out


def check_vacuumed(name, idx, st, top_level=False):
    """the statistics and the downloaded graph against the expected state; -> the lists"""
    case, D, R, links, new = expected(name)
    want_entry, want_mlv, changed = elected(case, top_level)
    print(f"vacuum {name}: stats {st}")
    assert st["dead_nodes"] == len(D) and st["nodes_repaired"] == len(R)
    assert st["dead_links_found"] == st["dead_links_dropped"] == links
    assert st["lists_written"] == len(new)
    assert (st["entry"], st["max_level"], st["entry_changed"]) == (want_entry, want_mlv, changed)
    (cnt, entry, mlv, levels), got = all_lists(case, idx)
    assert (cnt, entry, mlv) == (case.count, want_entry, want_mlv)
    assert np.array_equal(levels[1:cnt + 1], case.g.levels[1:cnt + 1])
    total = bad = 0
    for x in range(1, cnt + 1):
        assert len(got[x]) == len(case.lists[x]) or case.deleted[x]   # every level of every live node was looked at
        for l, lst in enumerate(got[x]):
            if case.deleted[x]:
                assert lst == [], (name, x, l)
            elif (x, l) in new:
                total += 1
                if lst != new[(x, l)]:
                    bad += 1
                    assert case.prec != I8, (name, x, l, lst, new[(x, l)])
                assert not any(is_dead_link(case, nb) for nb in lst), (name, x, l)
            else:
                assert lst == case.lists[x][l], (name, x, l)   # outside R: word for word as before
    print(f"vacuum {name}: {total} repaired lists compared, {bad} differed (rounding ties)")
    assert total == len(new) and bad <= max(2, total // 500), (name, bad, total)
    changed_lists = sum(1 for k, v in new.items() if v != case.lists[k[0]][k[1]])
    assert abs(st["lists_changed"] - changed_lists) <= bad
    return got


# ---- CPU: the census of the start graphs and the expected state itself ----------------------------------------------------------
CENSUS = {  # name: (nodes, |D|, |R|, dead links, entry, entry deleted, max_level, lowest live id, its level, top live level)
    "deleted": (3000, 750, 2250, 18323, 50, True, 2, 1, 0, 2),
    "few": (3000, 30, 726, 889, 959, True, 3, 1, 0, 3),
    "levels5": (1500, 75, 537, 730, 166, True, 4, None, None, 4),
    "f16": (800, 80, 708, 2159, None, False, None, None, None, None),
    "i8": (800, 80, 712, 2310, None, False, None, None, None, None),
}


@pytest.mark.parametrize("name", list(CENSUS))
def test_census_and_expected_state(oracle, name):
    """the start graphs are the ones the numbers of this file were made on (a changed generator shows here), and the expected
    state keeps its invariants: no live list names an id of D, no list holds its own node or a duplicate, len <= maxM"""
    case, D, R, links, new = expected(name)
    n, nd, nr, nl, entry, entry_dead, mlv, low, low_level, top = CENSUS[name]
    assert (case.count, len(D), len(R), links) == (n, nd, nr, nl)
    assert bool(case.deleted[case.g.entry]) == entry_dead
    if entry is not None:
        assert (case.g.entry, case.g.max_level) == (entry, mlv)
    live = [x for x in range(1, case.count + 1) if not case.deleted[x]]
    if low is not None:
        assert (live[0], int(case.g.levels[live[0]])) == (low, low_level)
    if top is not None:
        assert max(int(case.g.levels[x]) for x in live) == top
    if name == "levels5":                                       # dead links on the upper levels too
        assert sum(1 for x in R for lst in case.lists[x][1:] for nb in lst if is_dead_link(case, nb)) > 0
    assert {x for x, _ in new} == set(R) and R == sorted(R)
    assert len(new) == sum(len(case.lists[x]) for x in R)
    for x in live:
        for l, old in enumerate(case.lists[x]):
            lst = new.get((x, l), old)
            assert not any(is_dead_link(case, nb) for nb in lst), (x, l)
            assert x not in lst and len(set(lst)) == len(lst) and len(lst) <= case.maxm(l)


def test_helper_built_cases(oracle):
    case, D, R, links, new = expected("first3")
    assert D == sorted({1, 2, 3, case.g.entry}) and R and elected(case, False)[0] == 4
    case, D, R, links, new = expected("alldead")
    assert len(D) == case.count == 40 and not R and links == 0 and elected(case, False) == (0, -1, 1)


# ---- GPU --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["few", "levels5", "deleted", "cos"])
def test_dead_link_scan(oracle, hip, name):
    """test 1: the ids are R exactly, ascending; both counts exact; a cap below |R| still reports |R|; nothing is written"""
    case, D, R, links, _ = expected(name)
    idx = case.hip_index(hip)
    before = downloaded_lists(idx)
    ids, n_links, n_dead = idx.dead_link_scan()
    assert ids.tolist() == R and (n_links, n_dead) == (links, len(D))
    assert idx.last_scan_nodes == len(R)
    few, n_links, n_dead = idx.dead_link_scan(cap=min(5, len(R)))
    assert few.tolist() == R[:5] and idx.last_scan_nodes == len(R) and (n_links, n_dead) == (links, len(D))
    after = downloaded_lists(idx)
    assert before[0][:3] == after[0][:3] and np.array_equal(before[0][3], after[0][3]) and before[1] == after[1]
    assert after[1] == [[]] + case.lists[1:]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["few", "levels5"])
def test_vacuum_repairs_and_elects_by_the_reference_rule(oracle, hip, name):
    """test 2: R repaired list for list, D emptied, the 2244 live nodes of "few" outside R untouched (check_vacuumed compares
    every one of them word for word); the deleted entry is replaced by id 1 at level 0"""
    case, D, R, links, new = expected(name)
    idx = case.hip_index(hip)
    st = idx.vacuum(ef_construction=case.ef)
    assert (st["entry"], st["max_level"], st["entry_changed"]) == (1, 0, 1)
    if name == "few":
        assert case.count - len(D) - len(R) == 2244
    check_vacuumed(name, idx, st)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["deleted", "f16", "i8"])
def test_vacuum_every_live_node_and_a_live_entry(oracle, hip, name):
    """test 3: "deleted" -- every live node is repaired; "f16" / "i8" -- the entry point is alive and stays, max_level too;
    int8 lists are identical without exception"""
    case, D, R, links, new = expected(name)
    idx = case.hip_index(hip)
    st = idx.vacuum(ef_construction=case.ef)
    if name == "deleted":
        assert len(R) == case.count - len(D)
    else:
        assert (st["entry"], st["max_level"], st["entry_changed"]) == (case.g.entry, case.g.max_level, 0)
    check_vacuumed(name, idx, st)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["few", "levels5"])
def test_vacuum_elect_top_level(oracle, hip, name):
    """test 4: with the flag the entry is the lowest id among the live nodes of the top live level; the lists are those of the
    reference rule -- the flag changes header fields only"""
    case, D, R, links, new = expected(name)
    idx = case.hip_index(hip)
    st = idx.vacuum(ef_construction=case.ef, **ELECT_TOP)
    assert st["max_level"] == {"few": 3, "levels5": 4}[name] and st["entry_changed"] == 1
    assert not case.deleted[st["entry"]] and int(case.g.levels[st["entry"]]) == st["max_level"]
    assert not any(not case.deleted[x] and int(case.g.levels[x]) >= st["max_level"] for x in range(1, st["entry"]))
    got = check_vacuumed(name, idx, st, top_level=True)
    ref = case.hip_index(hip)
    st_ref = ref.vacuum(ef_construction=case.ef)
    assert all_lists(case, ref)[1] == got
    assert {k: v for k, v in st.items() if k not in ("entry", "max_level")} == {k: v for k, v in st_ref.items() if k not in ("entry", "max_level")}


@pytest.mark.gpu
def test_vacuum_elects_the_lowest_live_id(oracle, hip):
    """test 4, last point: ids 1..3 and the entry deleted -> without the flag the elected entry is id 4, with its own level"""
    case, D, R, links, new = expected("first3")
    idx = case.hip_index(hip)
    st = idx.vacuum(ef_construction=case.ef)
    assert (st["entry"], st["max_level"], st["entry_changed"]) == (4, int(case.g.levels[4]), 1)
    check_vacuumed("first3", idx, st)


@pytest.mark.gpu
def test_vacuum_cleanup(oracle, hip):
    """test 5: rows of D all zero bytes, live rows bit-identical, deleted bits and levels unchanged; with the half-precision
    ranking copy present an exact scan answers the same ids and distance bits before and after"""
    case, D, R, links, new = expected("few")
    idx = case.hip_index(hip)
    rng = np.random.default_rng(4)
    Q = (case.rows[rng.choice(np.arange(1, case.count + 1), 16, replace=False)] + 0.05 * rng.standard_normal((16, case.dim))).astype(np.float32)
    before = idx.flat_scan_batch(Q, 10)                         # (the first exact scan of a float32 index makes the ranking copy)
    rows0 = idx.download_rows(1, case.count)
    assert np.array_equal(rows0, case.rows[1:]) and all(rows0[d - 1].any() for d in D)
    st = idx.vacuum(ef_construction=case.ef, **ELECT_TOP)
    rows1 = idx.download_rows(1, case.count)
    dead = case.deleted[1:]
    assert not rows1[dead].view(np.uint8).any()
    assert np.array_equal(rows1[~dead].view(np.uint8), rows0[~dead].view(np.uint8))
    after = idx.flat_scan_batch(Q, 10)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[2], after[2])
    assert np.array_equal(before[1].view(np.uint32), after[1].view(np.uint32))
    assert not np.isin(after[0], np.array(D, dtype=np.uint32)).any()
    # the deleted bits: every id of D still has its bit (an exact scan allowed to see nothing but D finds nothing) and no other
    # id has one (the census counts |D| deleted nodes); levels: the downloaded table
    from kektordb_amd.index import dense_bitset
    only_d = idx.flat_scan_batch(Q, 10, allow_bits=dense_bitset(D, case.count))
    assert not only_d[2].any()
    assert idx.dead_link_scan()[2] == len(D)
    assert np.array_equal(idx.download_graph()[3][1:], case.g.levels[1:case.count + 1])


def _behaviour(fn):
    try:
        return ("ok",) + tuple(np.asarray(a).tobytes() for a in fn())
    except Exception as e:                                      # (whatever it is: the two indexes must agree on it)
        return ("raised", type(e).__name__)


@pytest.mark.gpu
def test_vacuum_with_everything_deleted(oracle, hip):
    """test 6: entry 0, max_level -1; searches behave exactly as on an index whose uploaded graph has max_level -1"""
    case, D, R, links, new = expected("alldead")
    idx = case.hip_index(hip)
    st = idx.vacuum(ef_construction=case.ef)
    assert (st["dead_nodes"], st["nodes_repaired"], st["lists_written"], st["dead_links_found"]) == (40, 0, 0, 0)
    assert (st["entry"], st["max_level"], st["entry_changed"]) == (0, -1, 1)
    assert idx.graph_info() == (case.count, 0, -1)
    assert not idx.download_rows(1, case.count).view(np.uint8).any()
    empty = hip.HipIndex(case.dim, case.metric, case.prec, case.m, case.ef, capacity=case.n + 8)
    empty.upload_rows(case.rows[1:], 1)
    empty.upload_graph(case.count, 0, -1, case.g.levels, case.g.offsets, case.g.neighbors, case.g.deleted_bits)
    assert empty.graph_info() == (case.count, 0, -1)
    Q = case.rows[1:9].astype(np.float32)
    for call in (lambda i: i.search_batch(Q, 10, 50), lambda i: i.flat_scan_batch(Q, 10),
                 lambda i: [len(i.SearchWithScores(Q[0], 5))]):
        assert _behaviour(lambda: call(idx)) == _behaviour(lambda: call(empty))
    again = idx.vacuum(ef_construction=case.ef)                # entry 0: the no-op
    assert not any(again.values()) and idx.graph_info() == (case.count, 0, -1)


@pytest.mark.gpu
def test_vacuum_is_idempotent_and_refuses_nothing_it_should_do(oracle, hip):
    """test 7: a second vacuum changes no adjacency word, no row, no header field and repairs 0 nodes; no deleted node: zero
    statistics, untouched graph; ef_construction 513 is refused and leaves the graph untouched"""
    case, D, R, links, new = expected("few")
    idx = case.hip_index(hip)
    start = all_lists(case, idx)
    with pytest.raises(hip.KdbError) as e:
        idx.vacuum(ef_construction=513)
    assert "status -" in str(e.value)
    same = all_lists(case, idx)
    assert same[0][:3] == start[0][:3] and same[1] == start[1] and same[1] == [[]] + case.lists[1:]
    assert np.array_equal(idx.download_rows(1, case.count), case.rows[1:])
    idx.vacuum(ef_construction=case.ef)
    first, rows = all_lists(case, idx), idx.download_rows(1, case.count)
    st = idx.vacuum(ef_construction=case.ef)
    assert (st["dead_nodes"], st["nodes_repaired"], st["lists_written"], st["lists_changed"]) == (len(D), 0, 0, 0)
    assert (st["dead_links_found"], st["dead_links_dropped"], st["entry_changed"]) == (0, 0, 0)
    assert (st["entry"], st["max_level"]) == first[0][1:3]
    second = all_lists(case, idx)
    assert second[0][:3] == first[0][:3] and np.array_equal(second[0][3], first[0][3]) and second[1] == first[1]
    assert np.array_equal(idx.download_rows(1, case.count).view(np.uint8), rows.view(np.uint8))
    clean = _vcase("cos")
    idx = clean.hip_index(hip)
    st = idx.vacuum(ef_construction=clean.ef)
    assert not any(st.values()), st
    (cnt, entry, mlv, _), lists = downloaded_lists(idx)
    assert (cnt, entry, mlv) == (clean.count, clean.g.entry, clean.g.max_level) and lists == [[]] + clean.lists[1:]
    assert idx.MaintenanceRun("vacuum") is False
    with pytest.raises(ValueError):
        idx.MaintenanceRun("compact")


@pytest.mark.gpu
def test_vacuum_is_scan_plus_refine_whatever_the_chunk(oracle, hip):
    """test 8: refine(ids = dead_link_scan ids) on a fresh copy gives the live nodes the lists vacuum gives them; and
    chunk_nodes 257 gives the graph of the default"""
    case, D, R, links, new = expected("few")
    a, b, c = case.hip_index(hip), case.hip_index(hip), case.hip_index(hip)
    assert a.MaintenanceRun("vacuum") is True                  # (the index's own efConstruction = case.ef)
    ids, _, _ = b.dead_link_scan()
    st = b.refine(ids, ef_construction=case.ef)
    assert st["nodes_refined"] == len(R) and st["dead_links_dropped"] == links
    la, lb = all_lists(case, a)[1], all_lists(case, b)[1]
    for x in range(1, case.count + 1):
        if not case.deleted[x]:
            assert la[x] == lb[x], x
        else:
            assert la[x] == [[] for _ in case.lists[x]] and lb[x] == case.lists[x]
    c.vacuum(ef_construction=case.ef, chunk_nodes=257)
    assert all_lists(case, c)[1] == la


@pytest.mark.gpu
@pytest.mark.parametrize("top_level", [False, True])
def test_search_after_vacuum_agrees_with_the_oracle(oracle, hip, top_level):
    """test 9: the walk over the vacuumed graph is the oracle's on the downloaded graph, bit for bit (64 queries); the entry is
    alive and no live list names an id of D, so no walk can reach a tombstone any more"""
    O = oracle
    case, D, R, links, new = expected("few")
    idx = case.hip_index(hip)
    idx.vacuum(ef_construction=case.ef, elect_top_level=top_level)
    cnt, entry, mlv, levels, offs, nbrs = idx.download_graph()
    assert (entry, mlv) == elected(case, top_level)[:2] and not case.deleted[entry]
    for l in range(mlv + 1):
        assert not case.deleted[nbrs[l]].any()
        src = np.repeat(np.arange(cnt + 1), np.diff(offs[l][:cnt + 2]).astype(np.int64))
        assert not case.deleted[src].any()                      # (and no deleted node has a link left to walk from)
    rows = np.zeros((cnt + 1, case.dim), dtype=np.float32)
    rows[1:] = idx.download_rows(1, cnt)
    g = O.Graph(cnt, levels, mlv, entry, offs, nbrs, case.g.deleted_bits)
    orc = O.OracleIndex.from_graph(case.dim, case.metric, case.prec, case.m, case.ef, rows, g)
    orc.set_arith(O.ARITH_HIP_WAVE)
    rng = np.random.default_rng(3)
    live = np.nonzero(~case.deleted[1:])[0] + 1
    Q = (case.rows[rng.choice(live, 64, replace=False)] + 0.05 * rng.standard_normal((64, case.dim))).astype(np.float32)
    ids, dist, c = idx.search_batch(Q, 10, 50)
    assert idx.counters()["n_dropped"] == 0
    for b in range(64):
        oi, od = orc.search(Q[b], 10, ef=50)
        assert np.array_equal(ids[b, :int(c[b])], oi), (b, ids[b], oi)
        assert np.array_equal(1.0 - dist[b, :int(c[b])].astype(np.float64), od)
