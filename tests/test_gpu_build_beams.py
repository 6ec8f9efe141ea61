"""build_search_kernel (kdb_index_add_batch, the fast builder) and refine_search_kernel (Refine, Vacuum) at every beam storage: the
cells of tests/walk_cells.py -- two register slots, four, the LDS beam, each boundary from both sides, for float32 L2, int8 cosine,
float32 cosine and float16 L2 -- with the protocols, helpers and pass conditions of test_gpu_build.py, test_gpu_refine.py and
test_gpu_vacuum.py.  Those modules walk with four register slots nowhere and with the LDS beam for float32 L2 (plus one int8 Refine
whose 450 live rows barely exceed its beam of 300).

Shapes: 48 columns, m = 4, clustered rows, forced levels, 1600 rows where the beam is in LDS and 800 below (walk_cells.py).
  * add_batch: test_add_batch_reference_links_list_for_list's protocol (test_gpu_build.add_batch_list_for_list): the oracle's first
    efConstruction single inserts go up as a graph, a tenth of them soft-deleted, the entry point among them; batches of 400 follow;
    every list of every level is compared after every batch.  int8: identical -- add_batch reports no ties, so nothing is excused
    (the rows are test_gpu_add_beams.py's: its tie control holds for them).  float32 / float16: max(2, lists // 500).
  * Refine: test_gpu_refine.Case with a tenth of the nodes soft-deleted, the entry point among them (4 % at efConstruction 256 and
    512: walk_cells.dead_for keeps 3 x efConstruction live rows); float32 refines every node, float16 / int8 a fixed subset of 200
    live ids in _subset's recipe (one replaced by a deleted id, one named twice) -- the Python layer search at ef 512 takes about
    15 ms per walk; every list outside the subset must be word for word as before (check_refined).
  * Vacuum: once, int8 at 512 with 160 of 1600 nodes deleted, against refine(ids of the scan) as
    test_vacuum_is_scan_plus_refine_whatever_the_chunk does it at ef 60.
  * the fast builder: float16 L2 at 200 and int8 cosine at 300, 1600 rows, built twice: bit-identical graphs, the list invariants of
    test_add_ties_are_reported, every row its own nearest with ef = efConstruction (distance 0; int8: the oracle's figure) -- the same
    asked of the oracle's own graph first, as the control, which is why these two cases have m = 16.
  * int8 at 512 once more behind poison_lds(0x5a5a5a5a), add_batch and Refine each.
  * "up" cases (walk_cells.UP_CELLS: m = 8, every second node raised): the only ones whose upper-layer walks reach more than
    KDB_UP_MARK_CAP nodes -- with m = 4 the entry point's island on level 1 holds 44 to 90 nodes.

Every case asserts from the oracle's data that it reaches its edges: kdb_walk_bs(efConstruction) is the storage it is named for; the
live rows number at least 3 x efConstruction and the oracle's level-0 walks return exactly efConstruction candidates (Refine:
facts["short0"] == 0); at least 384 nodes on level >= 1 where the beam is in LDS; deleted nodes present, the entry point among them,
and dead links met."""
import numpy as np
import pytest

import walk_cells as W
from test_gpu_add import assert_list_invariants, corpus, dense
from test_gpu_add_beams import POISON, OracleView, inputs
from test_gpu_build import add_batch_list_for_list
from test_gpu_refine import _case, _subset, check_invariants, check_refined, wide_rows
from test_gpu_vacuum import all_lists

pytestmark = pytest.mark.gpu

BATCH = 400


# ---- kdb_index_add_batch ------------------------------------------------------------------------------------------------------
def run_add_batch(O, hip, metric, prec, efc, poison=None, m=W.M, level_base=W.M):
    W.assert_walk_bs(efc)
    n, X, levels = inputs(O, prec, efc, level_base)
    r = add_batch_list_for_list(O, hip, metric, prec, X, levels, m, efc, (BATCH,) * 4, dead_frac=0.10, poison=poison)
    total, bad, orc, dead = r["total"], r["bad"], r["orc"], r["dead"]
    print(f"add_batch beams metric {metric} prec {prec} efc {efc} m {m} poison {poison}: {total} lists compared, {bad} differed (rounding ties)")
    assert r["added"] == n
    og = orc.export_graph()
    cnt = og.count - 1                                       # (the last reserved id holds no node, hnsw_index.go:1620)
    assert cnt == n - 1
    # the edges, from the oracle's data
    assert len(dead) == efc // 10 and cnt - len(dead) >= 3 * efc
    is_dead = np.zeros(og.count + 2, dtype=bool)
    is_dead[dead] = True
    od = dense(cnt, og.max_level, og.offsets, og.neighbors, None, m)
    assert is_dead[od[0][1:cnt + 1]].any()                   # dead links: walks go through deleted nodes, the side list is in play
    assert int(np.count_nonzero(od[0], axis=1).max()) == 2 * m
    og.count = cnt
    view = OracleView(orc, og, od, is_dead)
    wide = wide_rows(orc.rows(), prec, orc.absmax)
    for i in (cnt, cnt - 1, cnt - 100):                      # late nodes: the level-0 walk hands back a full beam
        assert len(view.walk(wide[i], og.entry, 0, efc)[0]) == efc, (efc, i)
    if efc > W.UP_MARK_CAP:
        upper = int(np.count_nonzero(og.levels[1:cnt + 1] >= 1))
        assert upper >= 384, upper
        far = W.reached(og, 1, og.entry)
        print(f"add_batch beams efc {efc} m {m}: {upper} nodes on level >= 1, {far} of them reached from the entry point")
        if m == W.UP_M:
            assert far > W.UP_MARK_CAP, far
            assert len(view.walk(wide[cnt], og.entry, 1, efc)[0]) > W.UP_MARK_CAP
    assert total > 3 * n // 4
    assert bad <= max(2, total // 500), (bad, total)
    if prec == O.I8:
        assert bad == 0


@pytest.mark.parametrize("name,metric,prec,efc", W.CELLS, ids=W.CELL_IDS)
def test_add_batch_cell(oracle, hip, name, metric, prec, efc):
    """one cell of build_search_kernel under the reference's own linking: list for list after every batch"""
    run_add_batch(oracle, hip, metric, prec, efc)


@pytest.mark.parametrize("name,metric,prec,efc", W.UP_CELLS, ids=W.UP_IDS)
def test_add_batch_upper_layer_marks_overflow(oracle, hip, name, metric, prec, efc):
    """m = 8, every second node on level >= 1: the upper-layer walks mark more than KDB_UP_MARK_CAP nodes"""
    run_add_batch(oracle, hip, metric, prec, efc, m=W.UP_M, level_base=W.UP_LEVEL_BASE)


def test_add_batch_int8_lds_beam_behind_poisoned_lds(oracle, hip):
    """int8 at efConstruction 512 with every CU's LDS filled with a finite pattern before each batch"""
    run_add_batch(oracle, hip, W.COSINE, W.I8, 512, poison=POISON)


# ---- the fast builder ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,metric,prec,efc", [("f16-l2", W.L2, W.F16, 200), ("i8-cos", W.COSINE, W.I8, 300)], ids=["f16-l2-200", "i8-cos-300"])
def test_fast_builder_wide_beams(oracle, hip, name, metric, prec, efc):
    """kdb_index_build with four register slots (float16) and with the LDS beam (int8): two builds give the same graph bit for bit,
    the lists keep their invariants, and every row is its own nearest neighbour when walked with ef = efConstruction -- which the
    oracle's own graph over the same rows is asked first.  m = 16 here: the control demands it (with m = 4 the oracle's own graph
    loses 652 of the 1600 float16 rows and 952 of the int8 rows, with m = 8 21 and 22, with m = 16 none).  The distance is 0 for
    float16; an int8 row that comes in as a float32 query is normalised and quantised again and stands up to 0.0026 from its stored
    form: there the device must give the oracle's figure, bit for bit."""
    O = oracle
    W.assert_walk_bs(efc)
    n, m = 1600, 16
    X = corpus(O, n, W.DIM, prec, 170, law="clustered")
    orc = O.OracleIndex(W.DIM, metric, prec, m, efc, seed=5)
    if prec == O.I8:
        orc.set_absmax(float(np.abs(X).max()))
    orc.set_arith(O.ARITH_HIP_WAVE)
    orc.add_many(X)
    rows = orc.rows()
    wide = wide_rows(rows, prec, orc.absmax)
    assert np.unique(rows[1:], axis=0).shape[0] == n, "two rows are equal once stored"
    own = np.zeros(n)
    for i in range(1, n + 1):                                # the control
        oi, dd = orc.search(wide[i], 1, ef=efc)
        assert len(oi) == 1 and oi[0] == i, ("control: the reference's own graph does not find node", i, oi, dd)
        own[i - 1] = dd[0]
    assert prec == O.I8 or not own.any()
    graphs = []
    for _ in range(2):
        idx = hip.HipIndex(W.DIM, metric, prec, m, efc, capacity=n + 8)
        idx.upload_rows(rows[1:], 1)
        if prec == O.I8:
            idx.upload_norms(orc.norms()[1:], 1)
            idx.set_quantizer(orc.absmax)
        idx.build(n, batch=BATCH, ef_construction=efc, seed=11)
        graphs.append(idx.download_graph())
    a, b = graphs
    assert a[:3] == b[:3] and a[0] == n and a[2] >= 1 and np.array_equal(a[3], b[3])
    for l in range(a[2] + 1):
        assert np.array_equal(a[4][l], b[4][l]) and np.array_equal(a[5][l], b[5][l]), l
    cnt, entry, mlv, glv, offs, nbrs = b
    assert 1 <= entry <= n and int(glv[entry]) == mlv
    assert_list_invariants(dense(cnt, mlv, offs, nbrs, None, m), cnt, glv[:cnt + 1], m)
    kw = {"dist64": True} if prec == O.I8 else {}
    ids, dist, c = idx.search_batch(wide[1:], 1, efc, **kw)
    assert np.all(c == 1) and np.array_equal(ids[:, 0], np.arange(1, n + 1))
    assert np.array_equal(dist[:, 0].astype(np.float64), own)


# ---- Refine and Vacuum ----------------------------------------------------------------------------------------------------------
def run_refine(hip, name, efc, poison=None, up=False, dead=""):
    W.assert_walk_bs(efc)
    case = _case(f"beam/{name}/{efc}/{dead}/{'up' if up else ''}")
    ids = None if case.prec == W.F32 else _subset(case, 200, live_only=True)
    new, facts = case.restate(ids)
    check_invariants(case, new, range(1, case.count + 1) if ids is None else ids)
    # the edges, from the oracle's data
    n_dead = int(case.deleted.sum())
    assert n_dead >= 32 and case.deleted[case.g.entry] and case.count - n_dead >= 3 * efc
    assert facts["short0"] == 0 and facts["dead"] > 0, facts
    if ids is not None:
        assert facts["nodes"] == 198 and case.deleted[ids].sum() == 1
    if efc > W.UP_MARK_CAP:
        upper = int(np.count_nonzero(case.g.levels[1:] >= 1))
        assert upper >= 384, upper
        far = W.reached(case.g, 1, case.g.entry)
        print(f"refine beams {name} efc {efc} up {up}: {upper} nodes on level >= 1, {far} of them reached from the entry point")
        if up:
            assert far > W.UP_MARK_CAP, far
    idx = case.hip_index(hip)
    if poison is not None:
        idx.poison_lds(poison)
    st = idx.refine(ids, ef_construction=efc)
    assert st["nodes_refined"] == facts["nodes"] and st["lists_written"] == len(new)
    assert st["dead_links_dropped"] == facts["dead"]
    total, bad = check_refined(case, idx, new, f"beam/{name}/{efc}")    # (every list outside `new` word for word as before)
    changed = sum(1 for k, v in new.items() if v != case.lists[k[0]][k[1]])
    assert abs(st["lists_changed"] - changed) <= bad
    return case, idx


@pytest.mark.parametrize("name,metric,prec,efc", W.CELLS, ids=W.CELL_IDS)
def test_refine_cell(oracle, hip, name, metric, prec, efc):
    """one cell of refine_search_kernel: every refined list against the restatement, every other list untouched"""
    case, _ = run_refine(hip, name, efc)
    assert (case.metric, case.prec, case.ef, case.m, case.dim) == (metric, prec, efc, W.M, W.DIM)


@pytest.mark.parametrize("name,metric,prec,efc", W.UP_CELLS, ids=W.UP_IDS)
def test_refine_upper_layer_marks_overflow(oracle, hip, name, metric, prec, efc):
    """m = 8, every second node on level >= 1: Refine walks its upper levels first "so that the bitset they un-mark is clean when
    level 0 starts" -- here they mark more than the un-mark list holds"""
    run_refine(hip, name, efc, up=True)


def test_refine_int8_lds_beam_behind_poisoned_lds(oracle, hip):
    """int8 at efConstruction 512 with every CU's LDS filled with a finite pattern before the call"""
    run_refine(hip, "i8-cos", 512, poison=POISON)


def test_vacuum_int8_lds_beam_is_scan_plus_refine(oracle, hip):
    """int8 at efConstruction 512, 160 of 1600 nodes deleted: refine(ids = dead_link_scan ids) on a fresh copy gives the live nodes
    the lists vacuum gives them, the deleted nodes' lists are emptied"""
    W.assert_walk_bs(512)
    case = _case("beam/i8-cos/512/160/")
    assert int(case.deleted.sum()) == 160 and case.deleted[case.g.entry]
    a, b = case.hip_index(hip), case.hip_index(hip)
    sa = a.vacuum(ef_construction=512)
    ids, links, n_dead = b.dead_link_scan()
    assert n_dead == 160 and links > 0 and ids.size > 0
    sb = b.refine(ids, ef_construction=512)
    assert sa["dead_nodes"] == 160 and sa["nodes_repaired"] == sb["nodes_refined"] == ids.size
    assert sa["dead_links_found"] == sa["dead_links_dropped"] == sb["dead_links_dropped"] == links
    assert sa["lists_written"] == sb["lists_written"] and sa["lists_changed"] == sb["lists_changed"]
    la, lb = all_lists(case, a)[1], all_lists(case, b)[1]
    for x in range(1, case.count + 1):
        if not case.deleted[x]:
            assert la[x] == lb[x], x
        else:
            assert la[x] == [[] for _ in case.lists[x]] and lb[x] == case.lists[x]
    repaired = set(ids.tolist())
    assert any(la[x] != case.lists[x] for x in repaired)
    assert all(la[x] == case.lists[x] for x in range(1, case.count + 1) if not case.deleted[x] and x not in repaired)
