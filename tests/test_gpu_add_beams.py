"""kdb_index_add / add_link_kernel<METRIC, BS, PREC> at every beam storage: the cells of tests/walk_cells.py (two register slots, four,
the LDS beam, each boundary from both sides) against the oracle's sequential Add, list for list, with test_gpu_add.py's helpers and
pass conditions.  test_gpu_add.py itself walks at efConstruction 24: two register slots and nothing else.

A case: 48 columns, m = 4, clustered rows, forced levels, 1600 rows where the beam is in LDS and 800 below; from an index without a
graph in calls of 1, 1, 5, 64 and then blocks of 200; after the first block 60 nodes are soft-deleted on both sides (32 at
efConstruction 256: walk_cells.dead_for), the entry point among them.  After EVERY call the header and every list of every level are
compared with the oracle's (ARITH_HIP_WAVE from its first add).

Pass conditions, the project's own:
  * headers equal, always;
  * float32 / float16: lists may differ by the pair-sum rounding ties of DESIGN 5.4, counted as test_add_float_per_node counts them
    (the oracle's graph goes up again after a differing call, so a tie is counted once) against max(2, lists // 500), lists = the
    lists the oracle's own adds changed, call by call;
  * int8: identical.  At these beam widths two earlier nodes can stand at EQUAL exact distance from a new one, and the walk orders
    equal distances by id where the oracle's heap does not: a call whose lists differ is excused only if the device itself reported
    tied_nodes > 0 for it; its graph must keep the list invariants, the oracle's graph goes up again, and the excused calls may
    cover at most 1 % of a case's nodes.  A differing int8 list with no tie reported fails.
    CPU control (tie_control, asserted per case): inserted nodes with two equal values among the efConstruction + 1 smallest
    orc.distances to the earlier live nodes.  With these seeds: 0 of 800 at efConstruction 128 and 129, 1 of 800 at 256, 3 of 1600 at
    257, 10 of 1600 at 512 (twelve row seeds gave 10 to 39 there: at a third of the corpus, equal int8 cosines are a property of such
    beams, and seed 192 is the lowest found).

Every case asserts from the oracle's data that it reaches its edges: kdb_walk_bs(efConstruction) is the storage the case is named for
(read from kdb_walk_lds.h through tests/cpp/walk_plan_test.cpp); the live rows number at least 3 x efConstruction and the oracle's
level-0 walk for late nodes returns exactly efConstruction candidates (a full beam that evicts); with the LDS beam at least 384 nodes
stand on level >= 1; reverse_pruned > 0; deleted nodes present and met by later walks.

384 upper nodes do NOT make an upper layer's walk mark more than the KDB_UP_MARK_CAP = 256 entries its un-mark list holds: with m = 4
the level-1 graph Add builds falls into islands and the entry point's holds 44 to 91 nodes (printed per case; walk_cells.py).  The
"up" cases (m = 8, every second node raised) are the ones that take VisBitset's full clear, on which add_link_kernel relies when it
lets "the levels below find the visited set clean": they assert that more than 256 nodes are reached from the entry point on level 1
and that the oracle's level-1 walk hands back more than 256 candidates."""
import numpy as np
import pytest

import walk_cells as W
from test_gpu_refine import Case, wide_rows
from test_gpu_add import (STAT_SUMS, assert_list_invariants, assert_same_header, corpus, draw_levels, gpu_add, gpu_dense, lists_differing,
                          new_pair, oracle_add, orc_dense)

pytestmark = pytest.mark.gpu

CALLS = (1, 1, 5, 64)
BLOCK = 200
DEAD_ASKED = 60
SEED_ROWS, SEED_LEVELS, SEED_DEAD = 192, 60, 161
POISON = 0x5a5a5a5a


def inputs(O, prec, efc, level_base=W.M):
    n = W.rows_for(efc)
    return n, corpus(O, n, W.DIM, prec, SEED_ROWS, law="clustered"), draw_levels(n, SEED_LEVELS, level_base)


class OracleView:
    """what Case.py_search_layer reads (searchLayerUnlocked restated in Python, every precision), over a pair's oracle"""
    def __init__(self, orc, og, dense_lists, is_dead):
        self.orc, self.count, self.deleted = orc, og.count, is_dead
        self.lists = [[dense_lists[l][x][dense_lists[l][x] != 0].tolist() for l in range(int(og.levels[x]) + 1)] for x in range(og.count + 1)]

    def walk(self, q, ep, level, ef):
        return Case.py_search_layer(self, q, ep, level, ef)


def call_sizes(n):
    sizes, pos = list(CALLS), sum(CALLS)
    while pos < n:
        sizes.append(min(BLOCK, n - pos))
        pos += sizes[-1]
    return sizes


def tie_control(orc, x, live, efc):
    """1 if two of the efc + 1 smallest distances from row x to the earlier live nodes are equal"""
    if len(live) < 2:
        return 0
    d = np.sort(orc.distances(x, np.asarray(live, dtype=np.uint32)))[:efc + 1]
    return int(np.any(d[1:] == d[:-1]))


def run_case(O, hip, metric, prec, efc, poison=None, m=W.M, level_base=W.M):
    W.assert_walk_bs(efc)
    n, X, levels = inputs(O, prec, efc, level_base)
    orc, idx = new_pair(O, hip, X, metric, prec, m, efc)
    n_dead = W.dead_for(n, efc, DEAD_ASKED)
    assert n_dead >= 32 and n - n_dead >= 3 * efc
    dead = np.zeros(0, dtype=np.uint32)
    is_dead = np.zeros(n + 2, dtype=bool)
    stats = {k: 0 for k in STAT_SUMS}
    pos = bad = total = excused = control = 0
    _, _, prev = orc_dense(orc, n + 1, m)
    for call, sz in enumerate(call_sizes(n)):
        lo, hi = pos + 1, pos + sz
        for i in range(lo, hi + 1):
            if prec == O.I8:
                control += tie_control(orc, X[i - 1], np.nonzero(~is_dead[1:i])[0] + 1, efc)
            oracle_add(orc, X, levels, i, i)
        if poison is not None:
            idx.poison_lds(poison)
        st = gpu_add(idx, orc, O, prec, levels, lo, hi, efc)
        for k in STAT_SUMS:
            stats[k] += st[k]
        og, oh, od = orc_dense(orc, n + 1, m)
        total += lists_differing(prev, od)                   # the lists the oracle's own adds changed
        prev = od
        gh, gd = gpu_dense(idx, n + 1, m)
        assert_same_header(gh, oh)
        assert (st["entry"], st["max_level"]) == oh[1:3]
        assert st["nodes_added"] == sz
        d = lists_differing(gd, od)
        if d and prec == O.I8:                               # only behind a tie the device itself reported
            assert st["tied_nodes"] > 0, (efc, call, sz, d, "int8 lists differ and no walk reported a tie")
            assert_list_invariants(gpu_dense(idx, None, m)[1], gh[0], gh[3], m)
            excused += sz
        elif d:                                              # a rounding tie: the next call starts from equal graphs again
            bad += d
        if d:
            idx.upload_graph_obj(og)
        pos = hi
        if call == len(CALLS):                               # behind the first block: the deletions
            rng = np.random.default_rng(SEED_DEAD)
            chosen = set(int(x) for x in rng.choice(np.arange(1, pos + 1), n_dead, replace=False))
            if orc.entry not in chosen:
                chosen.discard(next(iter(chosen)))
                chosen.add(orc.entry)
            dead = np.array(sorted(chosen), dtype=np.uint32)
            assert dead.size == n_dead and orc.entry in dead
            for x in dead:
                orc.mark_deleted(int(x))
            idx.Delete(dead)
            is_dead[dead] = True
            _, links, cnt_dead = idx.dead_link_scan()
            assert cnt_dead == n_dead and links > 0
    assert pos == n and stats["nodes_added"] == n
    print(f"add beams metric {metric} prec {prec} efc {efc} poison {poison}: {total} lists changed by the oracle's adds, {bad} differed "
          f"(rounding ties), {excused} nodes in excused calls, tie control {control}, stats {stats}")
    # the edges, from the oracle's data
    live = n - n_dead
    assert live >= 3 * efc
    view = OracleView(orc, og, od, is_dead)
    wide = wide_rows(orc.rows(), prec, orc.absmax)
    for i in (n, n - 1, n - 100):                            # late nodes: the level-0 walk hands back a full beam
        assert len(view.walk(wide[i], og.entry, 0, efc)[0]) == efc, (efc, i)
    assert stats["reverse_pruned"] > 0 and stats["reverse_appended"] > 0 and stats["reverse_skipped"] == 0
    assert idx.dead_link_scan()[2] == n_dead                 # the deleted nodes were there for every later walk
    for mat in gd:
        assert not is_dead[mat[sum(CALLS) + BLOCK + 1:]].any(), "a node added after the deletions names a deleted id"
    if efc > W.UP_MARK_CAP:
        upper = int(np.count_nonzero(oh[3][1:] >= 1))
        assert upper >= 384, upper
        far = W.reached(og, 1, og.entry)
        print(f"add beams efc {efc} m {m}: {upper} nodes on level >= 1, {far} of them reached from the entry point")
        if m == W.UP_M:                                      # a level-1 walk marks more than the un-mark list holds: full, or every node it reaches
            assert far > W.UP_MARK_CAP, far
            assert len(view.walk(wide[n], og.entry, 1, efc)[0]) > W.UP_MARK_CAP
    if prec == O.I8:
        assert control * 100 <= n, (control, n)
        assert excused * 100 <= n, (excused, n)
        assert bad == 0
    else:
        assert total >= n                                    # (every node's own level-0 list at the least)
        assert bad <= max(2, total // 500), (bad, total)
    return stats


@pytest.mark.parametrize("name,metric,prec,efc", W.CELLS, ids=W.CELL_IDS)
def test_add_cell(oracle, hip, name, metric, prec, efc):
    """one cell of add_link_kernel: after every call every list of every level against the oracle's"""
    run_case(oracle, hip, metric, prec, efc)


def test_add_int8_lds_beam_behind_poisoned_lds(oracle, hip):
    """int8 at efConstruction 512 -- 64-bit keys, the LDS beam with its *_lo array, the side list -- once more with every CU's LDS
    filled with a finite pattern before each call: a region the walk reads before it writes it shows as a wrong list"""
    run_case(oracle, hip, W.COSINE, W.I8, 512, poison=POISON)


@pytest.mark.parametrize("name,metric,prec,efc", W.UP_CELLS, ids=W.UP_IDS)
def test_add_upper_layer_marks_overflow(oracle, hip, name, metric, prec, efc):
    """m = 8, every second node on level >= 1 (walk_cells.UP_M): the upper-layer walks of efConstruction 512 mark more than
    KDB_UP_MARK_CAP nodes, the un-mark list overflows and the bitset is cleared whole before the level below walks"""
    run_case(oracle, hip, metric, prec, efc, m=W.UP_M, level_base=W.UP_LEVEL_BASE)
