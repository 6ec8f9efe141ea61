"""kdb_index_refine = GraphOptimizer.Refine / computeNewConnections (pkg/core/hnsw/optimizer.go:288-560) on the device.

The RESTATEMENT lives here and uses only what the oracle exports.  Per selected live node x and level l <= level(x):
  1. cand = searchLayerUnlocked(stored row of x, entry point, k = ef, level l, nil, ef) -- started on level l itself;
  2. + every current neighbour of x at l, in list order, that is not in cand, exists and is not deleted, at its node-to-node
     distance to x;   3. without x;   4. sorted by (distance, id) -- the library's rule where sort.Slice leaves ties open;
  5. selectNeighbors(.., mMax0 at level 0, m above) replaces the list.
Every list is computed from the graph as it was (phase 1, :354-410) before any is replaced (phase 2, :412-461).
float32: the oracle's own layer search (search_layer_raw).  float16 / int8: that export is float32-only, so searchLayerUnlocked
(hnsw_index.go:2351-2611) is restated in Python as tests/test_oracle_add_trace.py does, deleted nodes included (:2487, :2583-2590),
with orc.distances(widened row, ids, normalize_query=False) as the distance function.

Allowed differences (the condition of test_add_batch_reference_links_list_for_list): int8 lists are all identical; float32 /
float16 sum the pair distances inside selectNeighbors in another order than the oracle, so a list may differ where a pair
distance ties with a centre distance to rounding -- counted, printed, at most max(2, lists // 500) per case.  Lists refine
does not select must be bit-identical to before, always."""
import functools

import numpy as np
import pytest

from conftest import make_corpus
from test_oracle_add_trace import Heap

L2, COSINE = 0, 1
F32, F16, I8 = 0, 1, 2


# ---- corpora and start graphs (built once per process, never modified) -------------------------------------------------------
def wide_rows(rows, prec, absmax):
    """stored rows as the reference's queryObj: float32 as stored; float16 / int8 widened so that the oracle's conversion gives the
    stored row back"""
    if prec == F32:
        return rows
    if prec == F16:
        return rows.view(np.float16).astype(np.float32)
    return (rows.astype(np.float32) * np.float32(absmax)) / np.float32(127.0)


class Case:
    def __init__(self, O, metric, prec, n, dim, m, ef, seed, deleted_frac=0.0, delete_entry=False, law="clustered", level_cap=6,
                 level_base=None):
        self.O, self.metric, self.prec, self.n, self.dim, self.m, self.ef = O, metric, prec, n, dim, m, ef
        rng = np.random.default_rng(seed)
        X = make_corpus(n, dim, law, seed=seed + 1).astype(np.float32)
        if prec == F16:
            X = (X * 0.25).astype(np.float32)
        assert np.unique(X, axis=0).shape[0] == n              # no duplicate rows
        levels = np.minimum(np.floor(-np.log(1.0 - rng.random(n)) / np.log(level_base or m)), level_cap).astype(np.int32)
        orc = O.OracleIndex(dim, metric, prec, m, ef, seed=5)
        if prec == I8:
            orc.set_absmax(float(np.abs(X).max()))
        for i in range(n):
            orc.add(X[i], level=int(levels[i]))
        if deleted_frac:
            dead = rng.choice(np.arange(1, n + 1), int(n * deleted_frac), replace=False).tolist()
            if delete_entry and orc.entry not in dead:
                dead[0] = orc.entry
            for d in dead:
                orc.mark_deleted(int(d))
        orc.set_arith(O.ARITH_HIP_WAVE)
        self.orc = orc
        self.rows = orc.rows()
        self.norms = orc.norms()
        self.g = orc.export_graph()
        self.count = self.g.count
        assert self.count == n
        db = self.g.deleted_bits
        self.deleted = np.array([(int(db[i >> 6]) >> (i & 63)) & 1 for i in range(n + 1)], dtype=bool)
        self.lists = [[self._list(l, x) for l in range(int(self.g.levels[x]) + 1)] for x in range(n + 1)]   # [node][level]
        self.wide = wide_rows(self.rows, prec, orc.absmax)
        self._restated = {}

    def _list(self, l, x):
        off = self.g.offsets[l]
        return self.g.neighbors[l][int(off[x]):int(off[x + 1])].tolist()

    def maxm(self, l):
        return 2 * self.m if l == 0 else self.m

    # -- searchLayerUnlocked (hnsw_index.go:2351-2611) in Python, for the precisions search_layer_raw does not take
    def py_search_layer(self, q, ep, level, ef):
        dist = lambda ids: self.orc.distances(q, ids, normalize_query=False)
        visited = {ep}
        cands, results = Heap(False), Heap(True)
        e = (ep, float(dist([ep])[0]))
        cands.push(e)
        if not self.deleted[ep]:                                # :2487
            results.push(e)
        while cands.a:
            cur = cands.pop()
            if len(results.a) >= ef and cur[1] > results.a[0][1]:   # :2501-2506
                break
            cl = self.lists[cur[0]]
            if level >= len(cl):                                # :2521
                continue
            fresh = []
            for nb in cl[level]:
                if nb in visited:
                    continue
                visited.add(nb)
                if 1 <= nb <= self.count:
                    fresh.append(nb)
            if not fresh:
                continue
            for nb, d in zip(fresh, dist(fresh).tolist()):
                worst = results.a[0][1] if results.a else 1.7976931348623157e308
                if len(results.a) < ef or d < worst:            # :2577
                    cands.push((nb, d))
                    if not self.deleted[nb]:                    # :2583-2590
                        results.push((nb, d))
                        if len(results.a) > ef:
                            results.pop()
        out = [None] * len(results.a)
        for i in range(len(results.a) - 1, -1, -1):
            out[i] = results.pop()
        return np.array([c[0] for c in out], dtype=np.uint32), np.array([c[1] for c in out], dtype=np.float64)

    def restate(self, ids=None, ef=None):
        """-> ({(node, level): new list}, facts) for Refine over `ids` (None: every node) on the start graph"""
        ef = ef or self.ef
        key = (None if ids is None else tuple(int(i) for i in ids), ef)
        if key in self._restated:
            return self._restated[key]
        sel = range(1, self.count + 1) if ids is None else ids
        new, facts = {}, {"cur": 0, "appended": 0, "merged_lists": 0, "dead": 0, "short": 0, "short0": 0, "nodes": 0}
        for x in dict.fromkeys(int(i) for i in sel):            # a node named twice: once (same snapshot, same result)
            if self.deleted[x]:                                 # optimizer.go:341
                continue
            facts["nodes"] += 1
            q = self.wide[x]
            for l in range(int(self.g.levels[x]) + 1):
                if self.prec == F32:
                    cid, cd = self.orc.search_layer_raw(q, self.g.entry, ef, l, ef)
                else:
                    cid, cd = self.py_search_layer(q, self.g.entry, l, ef)
                if len(cid) >= 2 and len(cid) == ef:            # no distance tie at the ef boundary
                    assert cd[-1] != cd[-2], (x, l)
                assert not self.deleted[cid].any()
                if len(cid) < ef:
                    facts["short"] += 1
                    facts["short0"] += int(l == 0)              # (level 0 alone: the beam-storage cases ask for a full beam there)
                have = set(cid.tolist())
                extra = []
                for nb in self.lists[x][l]:                     # :497-522
                    facts["cur"] += 1
                    if not (1 <= nb <= self.count) or self.deleted[nb]:
                        facts["dead"] += 1
                        continue
                    if nb in have:
                        continue
                    have.add(nb)
                    extra.append(nb)
                facts["appended"] += len(extra)
                facts["merged_lists"] += 1 if extra else 0
                if extra:
                    cid = np.concatenate([cid, np.array(extra, dtype=np.uint32)])
                    cd = np.concatenate([cd, self.orc.distances(q, extra, normalize_query=False)])
                keep = cid != x                                 # :524-536
                cid, cd = cid[keep], cd[keep]
                order = np.lexsort((cid, cd))                   # (distance, id)
                new[(x, l)] = self.orc.select_neighbors(cid[order], cd[order], self.maxm(l)).tolist()
        self._restated[key] = (new, facts)
        return new, facts

    # -- the GPU side
    def hip_index(self, hip):
        idx = hip.HipIndex(self.dim, self.metric, self.prec, self.m, self.ef, capacity=self.n + 8)
        idx.upload_rows(self.rows[1:], 1)
        if self.prec == I8:
            idx.upload_norms(self.norms[1:], 1)
            idx.set_quantizer(self.orc.absmax)
        idx.upload_graph_obj(self.g)
        return idx


def downloaded_lists(idx):
    cnt, entry, mlv, levels, offs, nbrs = idx.download_graph()
    out = [[] for _ in range(cnt + 1)]
    for x in range(1, cnt + 1):
        for l in range(int(levels[x]) + 1):
            out[x].append(nbrs[l][int(offs[l][x]):int(offs[l][x + 1])].tolist())
    return (cnt, entry, mlv, levels), out


def check_refined(case, idx, new, label):
    """the downloaded graph against the start graph with `new` put in; -> (refined lists compared, lists that differ)"""
    (cnt, entry, mlv, levels), got = downloaded_lists(idx)
    assert (cnt, entry, mlv) == (case.count, case.g.entry, case.g.max_level)
    assert np.array_equal(levels[1:cnt + 1], case.g.levels[1:cnt + 1])
    total = bad = 0
    for x in range(1, cnt + 1):
        for l in range(int(levels[x]) + 1):
            want = new.get((x, l))
            if want is None:                                    # not selected (or deleted): untouched
                assert got[x][l] == case.lists[x][l], (label, x, l)
                continue
            total += 1
            if got[x][l] != want:
                bad += 1
                assert case.prec != I8, (label, x, l, got[x][l], want)
    print(f"refine {label}: {total} lists compared, {bad} differed (rounding ties)")
    assert bad <= max(2, total // 500), (label, bad, total)
    return total, bad


def check_invariants(case, new, selected):
    live_sel = {int(x) for x in selected if not case.deleted[int(x)]}
    assert {x for x, _ in new} == live_sel
    for (x, l), lst in new.items():
        assert len(lst) <= case.maxm(l)
        assert x not in lst
        assert len(set(lst)) == len(lst)
        assert not any(case.deleted[nb] for nb in lst)
        assert all(1 <= nb <= case.count for nb in lst)


@functools.lru_cache(maxsize=None)
def _case(name):
    from oracle import oracle as O
    O.build()
    if name.startswith("beam/"):            # "beam/<cell>/<efConstruction>[/<deleted nodes>[/up]]": a cell of tests/walk_cells.py; up: its wide upper layers
        import walk_cells as W
        part = name.split("/") + ["", ""]
        metric, prec = {c[0]: c[1:3] for c in W.CELLS}[part[1]]
        efc = int(part[2])
        n = W.rows_for(efc)
        dead = int(part[3]) if part[3] else W.dead_for(n, efc, n // 10)
        m, base = (W.UP_M, W.UP_LEVEL_BASE) if part[4] == "up" else (W.M, None)
        return Case(O, metric, prec, n, W.DIM, m, efc, seed=BEAM_SEED, deleted_frac=(dead + 0.5) / n, delete_entry=True, level_base=base)
    mk = {
        "cos": lambda: Case(O, COSINE, F32, 3000, 96, 16, 60, seed=11),
        "l2": lambda: Case(O, L2, F32, 3000, 96, 16, 60, seed=12),
        "levels": lambda: Case(O, L2, F32, 1500, 64, 4, 8, seed=13, level_cap=4),
        "deleted": lambda: Case(O, COSINE, F32, 3000, 96, 16, 60, seed=11, deleted_frac=0.25, delete_entry=True),
        "tiny": lambda: Case(O, COSINE, F32, 40, 96, 16, 60, seed=14),
        "one": lambda: Case(O, COSINE, F32, 1, 96, 16, 60, seed=15, law="normal"),
        "lds": lambda: Case(O, L2, F32, 1500, 64, 16, 400, seed=16),
        "odd": lambda: Case(O, L2, F32, 1000, 200, 16, 60, seed=17),
        "f16": lambda: Case(O, L2, F16, 800, 96, 16, 32, seed=18, deleted_frac=0.10),
        "i8": lambda: Case(O, COSINE, I8, 800, 96, 16, 32, seed=19, deleted_frac=0.10),
        # every region of a walking wave's LDS live at once: 64-bit keys (the *_lo arrays), the LDS beam (ef > 256), the side list
        "i8lds": lambda: Case(O, COSINE, I8, 500, 96, 16, 300, seed=20, deleted_frac=0.10),
    }
    return mk[name]()


BEAM_SEED = 30


def _subset(case, k=300, live_only=False):
    rng = np.random.default_rng(5)
    pool = np.nonzero(~case.deleted[1:])[0] + 1 if live_only else np.arange(1, case.count + 1)
    ids = rng.choice(pool, k, replace=False).astype(np.uint32)
    dead = np.nonzero(case.deleted)[0]
    if not case.deleted[ids].any():
        ids[7] = dead[0]
    ids[11] = ids[3]                                            # a duplicate
    return ids


# ---- CPU: the checker itself --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["deleted", "tiny", "one"])
def test_restated_refine_keeps_its_invariants(oracle, name):
    """the restatement alone (no GPU): every new list has at most maxM entries, never its own node, no duplicate, no deleted
    id; lists of nodes that were not selected are not produced at all"""
    case = _case(name)
    new, facts = case.restate()
    check_invariants(case, new, range(1, case.count + 1))
    if name == "deleted":
        assert case.deleted[case.g.entry] and int(case.deleted.sum()) == 750
        assert facts["dead"] > 1000                            # the start graph really held dead links
        sub = _subset(case)
        assert case.deleted[sub].any() and len(set(sub.tolist())) < len(sub)
        new_s, _ = case.restate(sub)
        check_invariants(case, new_s, sub)
        assert all(new_s[k] == new[k] for k in new_s)           # a subset gives the same lists: same snapshot
    if name == "tiny":
        assert facts["short"] == len(new)                       # fewer candidates than ef everywhere
    if name == "one":
        assert new == {(1, l): [] for l in range(int(case.g.levels[1]) + 1)}


def test_int8_widened_row_quantises_back(oracle):
    """the int8 restatement hands the oracle q8 * absmax / 127 as the query: quantising that must give the stored row"""
    case = _case("i8")
    a = np.float32(case.orc.absmax)
    scaled = np.clip((case.wide / a).astype(np.float32) * np.float32(127.0), -127.0, 127.0).astype(np.float64)
    back = (np.sign(scaled) * np.floor(np.abs(scaled) + 0.5)).astype(np.int8)   # C round(): half away from zero
    assert np.array_equal(back, case.rows) and case.rows.any()


# ---- GPU --------------------------------------------------------------------------------------------------------------------
def _refine_all(hip, name, **kw):
    case = _case(name)
    new, facts = case.restate()
    idx = case.hip_index(hip)
    st = idx.refine(ef_construction=case.ef, **kw)
    assert st["nodes_refined"] == facts["nodes"] and st["lists_written"] == len(new)
    assert st["dead_links_dropped"] == facts["dead"]
    total, bad = check_refined(case, idx, new, name)
    changed = sum(1 for k, v in new.items() if v != case.lists[k[0]][k[1]])
    assert abs(st["lists_changed"] - changed) <= bad
    return case, idx, new, facts


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cos", "l2"])
def test_refine_f32_list_for_list(oracle, hip, name):
    """case 1: n 3000, dim 96, m 16, ef 60, graph from the oracle's add; every list of every node equals the restatement's"""
    _refine_all(hip, name)


@pytest.mark.gpu
def test_refine_many_levels_and_the_merge_path(oracle, hip):
    """case 2: m 4, ef 8 on five populated levels.  ef equals mMax0 and x is one of its own ef candidates, so a full level-0 list
    can never be wholly among them: most lists reach the union through the merge (membership test, extra distances).  Measured
    on the oracle: 43 % of all current neighbours are appended that way (not "most neighbours" -- the walk from the entry point
    still finds the others), in more than half of the lists."""
    case, idx, new, facts = _refine_all(hip, "levels")
    assert case.g.max_level >= 2 and all(np.count_nonzero(case.g.levels[1:] >= l) >= 3 for l in range(3))
    assert facts["merged_lists"] * 2 > len(new) and facts["appended"] * 3 > facts["cur"], facts


@pytest.mark.gpu
def test_refine_with_deleted_nodes(oracle, hip):
    """case 3: a quarter of the nodes deleted, the entry point among them: no live list keeps a deleted id, the dropped dead
    links are counted, deleted nodes keep their lists"""
    case, idx, new, facts = _refine_all(hip, "deleted")
    (_, _, _, levels), got = downloaded_lists(idx)
    for x in range(1, case.count + 1):
        for l, lst in enumerate(got[x]):
            if case.deleted[x]:
                assert lst == case.lists[x][l]
            else:
                assert not any(case.deleted[nb] for nb in lst), (x, l)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["tiny", "one"])
def test_refine_tiny_graphs(oracle, hip, name):
    """case 4: fewer nodes than ef (every walk returns fewer than ef candidates); a single node keeps an empty list"""
    case, idx, new, facts = _refine_all(hip, name)
    if name == "one":
        assert downloaded_lists(idx)[1][1] == [[] for _ in range(int(case.g.levels[1]) + 1)]


@pytest.mark.gpu
def test_refine_lds_beam(oracle, hip):
    """case 5: ef 400 -- the beam of the walk lives in LDS"""
    _refine_all(hip, "lds")


@pytest.mark.gpu
def test_refine_odd_row_length(oracle, hip):
    """case 6: dim 200 is no multiple of the 128-float K-chunk of selectNeighbors"""
    _refine_all(hip, "odd")


@pytest.mark.gpu
def test_refine_subset_and_bad_ids(oracle, hip):
    """case 7: 300 ids with a duplicate and a deleted one: only those lists change, every other adjacency word is as before;
    an id of 0 or count + 1 is refused and leaves the graph unchanged"""
    case = _case("deleted")
    ids = _subset(case)
    new, facts = case.restate(ids)
    idx = case.hip_index(hip)
    before = downloaded_lists(idx)[1]
    for bad_id in (0, case.count + 1):
        with pytest.raises(hip.KdbError) as e:
            idx.refine(np.concatenate([ids[:5], np.array([bad_id], dtype=np.uint32)]), ef_construction=case.ef)
        assert "status -" in str(e.value)
        assert downloaded_lists(idx)[1] == before
    assert before == [[]] + case.lists[1:]
    st = idx.refine(ids, ef_construction=case.ef)
    assert st["nodes_refined"] == facts["nodes"] == len(set(ids.tolist())) - int(case.deleted[np.unique(ids)].sum())
    assert st["lists_written"] == len(new) and st["dead_links_dropped"] == facts["dead"]
    check_refined(case, idx, new, "subset")                     # (asserts every list outside `new` is untouched)


@pytest.mark.gpu
def test_refine_is_a_snapshot_whatever_the_chunk(oracle, hip):
    """case 8: chunk_nodes 257 and the default give identical graphs, two runs from the same start are identical, and both are
    the restatement computed on the SNAPSHOT -- an implementation that commits as it goes differs from it on case 1"""
    case = _case("cos")
    new, _ = case.restate()
    graphs = []
    for kw in ({}, {"chunk_nodes": 257}, {}):
        idx = case.hip_index(hip)
        idx.refine(ef_construction=case.ef, **kw)
        graphs.append(downloaded_lists(idx)[1])
        if len(graphs) == 2:
            check_refined(case, idx, new, "chunk 257")
        idx.close()
    assert graphs[0] == graphs[1] == graphs[2]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["f16", "i8", "i8lds"])
def test_refine_f16_and_int8(oracle, hip, name):
    """case 9: float16 (L2) and int8 (cosine), a tenth of the nodes deleted; int8 lists are identical without exception
    (i8lds: int8 at ef 300, the beam in LDS)"""
    _refine_all(hip, name)


@pytest.mark.gpu
def test_search_after_refine_agrees_with_the_oracle(oracle, hip):
    """case 10: the walk over the lists refine wrote is still the oracle's, bit for bit (64 queries), and RunTurboRefine clears
    needs_refine (optimizer.go:716)"""
    O = oracle
    case = _case("cos")
    idx = case.hip_index(hip)
    idx.needs_refine = True
    st = idx.RunTurboRefine()
    assert idx.needs_refine is False and st["nodes_refined"] == case.count
    cnt, entry, mlv, levels, offs, nbrs = idx.download_graph()
    g = O.Graph(cnt, levels, mlv, entry, offs, nbrs, case.g.deleted_bits)
    orc = O.OracleIndex.from_graph(case.dim, case.metric, case.prec, case.m, case.ef, case.rows, g)
    orc.set_arith(O.ARITH_HIP_WAVE)
    rng = np.random.default_rng(3)
    Q = (case.rows[rng.choice(np.arange(1, cnt + 1), 64, replace=False)] + 0.05 * rng.standard_normal((64, case.dim))).astype(np.float32)
    ids, dist, c = idx.search_batch(Q, 10, 50)
    for b in range(64):
        oi, od = orc.search(Q[b], 10, ef=50)
        assert np.array_equal(ids[b, :int(c[b])], oi), (b, ids[b], oi)
        assert np.array_equal(1.0 - dist[b, :int(c[b])].astype(np.float64), od)
