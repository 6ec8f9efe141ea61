"""Query preparation at its edge values, through BOTH copies of it, and the distance tile that lets a test look at a prepared query.

searchInternal prepares a query before anything compares it with a row (hnsw_index.go:404-434): cosine normalisation in normalize()'s
order, the float16 round trip, Quantizer.Quantize and the int8 query norm.  The device holds that code twice:

  prep_queries_kernel (search.hip)                    kdb_load_query, the raw branch (kdb_search_core.cuh)
  ------------------------------------------------    ------------------------------------------------------------
  kdb_distance_batch[_dev]        every precision     kdb_search_batch[_dev / _mixed / _multi]   float32, float16
  kdb_flat_scan_batch[_dev], _groups_dev    "         kdb_search_by_id[_dev]                     float32, float16
  kdb_flat_scan_by_id[_dev]                 "         (KDB_SEARCH_HEAP_ORDER re-walks with the same function)
  kdb_search_filtered, its scanned queries  "
  every graph search of an int8 index (its walk then loads the quantised copy and the norm)

WHAT IS COMPARED.  Section 1 looks at the prepared query one element at a time: probe rows (unit vectors, a zero row, 127 * e_i) make
a distance BE an element of the prepared query, and a numpy restatement of the reference (query_prep_ref.py) or the oracle says
what it must be.  Section 2 holds the distance tile to the oracle in its four instantiations at the chunk boundary of 32 candidates.
Section 3 holds walk, heap-order walk, exact scan, by-id calls and the distance tile to one answer per (query, row).  Every
comparison is on bits or exact counts; the only freedom is the sign of a zero in section 1 (q_i * 1 + 0 * 0 turns -0.0 into +0.0).

ONE RULE for a query that is not finite ONCE PREPARED (include/kektor_hip.h, "Conventions"): count 0, ids 0 and +Inf from
every search and scan, +Inf for every candidate from the distance tile.  From finite values only a float16 index produces one (a
component of 65520 or more): float32 normalisation cannot (a sum of squares that overflows gives the inverse 0 and the query zeros;
inf * 0 needs an infinity in the caller's values).

TIES.  The fast walk orders equal distances by id, the reference by heap history (search.hip, header); only KDB_SEARCH_HEAP_ORDER
promises the reference's ids then.  A query that is equally far from two rows of the index (decided with the oracle's distances to
every row, before anything runs on the device) is therefore held to the oracle's ids only under heap order; without it, and in
the exact scan, its distances and its (query, id) pairs are still checked."""
import numpy as np
import pytest

from conftest import make_corpus
from query_prep_ref import (COSINE, F16, F32, I8, L2, QUANT_A, f16_edge_values, f32_query_pool, i8_query_values, np_f16_round_trip,
                            np_normalize, np_prepared, same_bits)
from test_gpu_compress_edges import bare_graph
from test_gpu_parity import build_pair

CELLS = [(L2, F32), (COSINE, F32), (L2, F16), (COSINE, I8)]     # the four instantiations of distance_tile_kernel
HEAP = {"heap_order": True, "tie_flag": True}
COUNT_MASK = 0x7fffffff


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def score(metric, prec, raw):
    """the reference's float64 epilogue of a raw float32 answer (HipIndex.score, vectorised)"""
    raw = np.asarray(raw, dtype=np.float64)
    return 1.0 - raw if (prec == F32 and metric == COSINE) else raw


def all_ids(B, n):
    return np.tile(np.arange(1, n + 1, dtype=np.uint32), (B, 1))


# ---- 0. no GPU: the two references against each other, the pools' own claims --------------------------------------------------------
@pytest.mark.parametrize("dim", [3, 16, 70, 100, 768])
def test_numpy_normalize_is_the_oracles(oracle, dim):
    """np_normalize against the oracle's restatement of normalize(), through unit-vector rows: the oracle's distance to e_i is
    1 - float64(component i).  The pools' own claims are asserted where the pools are made."""
    O = oracle
    rows = np.zeros((dim + 1, dim), np.float32)
    rows[1:] = np.eye(dim, dtype=np.float32)
    orc = O.OracleIndex.from_graph(dim, COSINE, F32, 8, 40, rows, bare_graph(O, dim, []))
    orc.set_arith(O.ARITH_HIP_WAVE)
    for nm, q in f32_query_pool(dim).items():
        want = 1.0 - np_normalize(q).astype(np.float64)
        assert np.array_equal(orc.distances(q, np.arange(1, dim + 1)), want), (dim, nm)
    f16_edge_values()
    i8_query_values()
    for metric, prec in CELLS:
        section3_queries(metric, prec, dim)


# ---- 1. the prepared query, element by element -------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dim", [3, 16, 70, 100, 768])
def test_float32_cosine_query_element_by_element(oracle, hip, dim):
    """Rows e_1..e_dim: the raw answer for (q, e_i) is the normalised q_i exactly (every other product is with 0).  The distance tile
    shows prep_queries_kernel (B and dim off its 16-query and 64-column tiles), a walk shows kdb_load_query (dim % 4 != 0: its scalar
    tail loop; 3 queries: four waves each, 300: one)."""
    E = np.eye(dim, dtype=np.float32)
    orc, idx = build_pair(oracle, hip, E, COSINE, m=8, efc=40)
    assert np.array_equal(bits(idx.download_rows(1, dim)), bits(E))                     # stored unchanged
    pool = f32_query_pool(dim)
    names = list(pool)
    P = np.stack([pool[nm] for nm in names])
    want = np.stack([np_normalize(q) for q in P])
    assert np.isfinite(want).all()
    ids = all_ids(33, dim)
    for B in (1, 15, 16, 17, 33):
        for shift in (range(len(names)) if B == 1 else (0, 4)):
            sel = (np.arange(B) + shift) % len(names)
            got = idx.distance_batch(P[sel], ids[:B])
            for r, p in enumerate(sel):
                assert same_bits(got[r], want[p]), ("distance tile", dim, B, r, names[p], np.nonzero(got[r] != want[p])[0][:4])
    k = min(dim, 32)
    for B, kw in ((3, {}), (3, HEAP), (300, {})):
        for shift in (0, 3, 6) if B == 3 else (0,):
            sel = (np.arange(B) + shift) % len(names)
            sid, sd, sc = idx.search_batch(P[sel], k, 64, **kw)
            for r, p in enumerate(sel):
                c = int(sc[r]) & COUNT_MASK
                assert 1 <= c <= k and np.all(sid[r, :c] >= 1) and np.all(sid[r, :c] <= dim), (dim, B, r, names[p])
                assert same_bits(sd[r, :c], want[p][sid[r, :c].astype(np.int64) - 1]), ("walk", dim, B, kw, r, names[p])


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [16, 70])
def test_float16_query_element_by_element(oracle, hip, dim):
    """One zero row and queries c * e_i: the L2 answer is float32(float16(c)) squared, exactly (the square of a half has 22
    significant bits).  np.float16 is the reference."""
    c = f16_edge_values()
    B = c.size
    idx = hip.HipIndex(dim, L2, F16, 8, 40, capacity=8)
    idx.upload_rows(np.zeros((1, dim), np.uint16), 1)
    idx.upload_graph_obj(bare_graph(oracle, 1, []))
    Q = np.zeros((B, dim), np.float32)
    Q[np.arange(B), np.arange(B) % dim] = c
    h = np_f16_round_trip(c)
    want = h * h
    assert want.dtype == np.float32 and np.array_equal(want.astype(np.float64), h.astype(np.float64) ** 2)
    got = idx.distance_batch(Q, np.ones((B, 1), np.uint32))[:, 0]
    assert np.array_equal(bits(got), bits(want)), ("distance tile", c[bits(got) != bits(want)])
    chunks = [slice(0, B)] + [slice(a, a + 3) for a in range(0, B, 3)]                  # one call, then three queries at a time
    for kw in ({}, HEAP):
        for sl in chunks:
            sid, sd, sc = idx.search_batch(Q[sl], 1, 10, **kw)
            assert np.all((sc & COUNT_MASK) == 1) and np.all(sid[:, 0] == 1), (dim, kw, sl)
            assert np.array_equal(bits(sd[:, 0]), bits(want[sl])), ("walk", kw, sl, c[sl][bits(sd[:, 0]) != bits(want[sl])])


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [16, 70, 768])
def test_float16_dense_queries_match_the_oracle(oracle, hip, dim):
    O = oracle
    n = 40
    orc, idx = build_pair(O, hip, make_corpus(n, dim, "normal", seed=31), L2, precision=F16, m=8, efc=40)
    orc.set_arith(O.ARITH_HIP_WAVE)
    rng = np.random.default_rng(dim)
    c = f16_edge_values()
    Q = np.concatenate([rng.standard_normal((17, dim)).astype(np.float32) * np.float32(3.0),
                        np.resize(rng.permutation(c), 4 * dim).reshape(4, dim).astype(np.float32)])
    got = idx.distance_batch(Q, all_ids(Q.shape[0], n))
    for b in range(Q.shape[0]):
        assert np.array_equal(got[b].astype(np.float64), orc.distances(Q[b], np.arange(1, n + 1))), (dim, b)


def int8_probe(O, hip, dim, absmax):
    """rows 127 * e_i with their norms, no graph: (oracle, device index)"""
    rows = np.zeros((dim + 1, dim), np.int8)
    rows[1:] = 127 * np.eye(dim, dtype=np.int8)
    norms = np.zeros(dim + 1, np.float32)
    norms[1:] = 127.0
    orc = O.OracleIndex.from_graph(dim, COSINE, I8, 8, 40, rows, bare_graph(O, dim, []), norms=norms, absmax=float(absmax))
    idx = hip.HipIndex(dim, COSINE, I8, 8, 40, capacity=dim + 8)
    idx.upload_rows(rows[1:], 1)
    idx.upload_norms(norms[1:], 1)
    idx.set_quantizer(float(absmax))
    idx.set_count(dim)
    return orc, idx


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [20, 70])
def test_int8_query_element_by_element(oracle, hip, dim):
    """Rows 127 * e_i.  A two-hot query (c at one place, A at the last) quantises to (q_c, 127): its distance to e_i is
    1 - 127 q_c / (127 sqrt(q_c^2 + 127^2)), strictly monotone in q_c -- one wrong rounding of c shows.  Normalisation is kept out
    with KDB_SEARCH_PREPARED, which the ABI accepts for int8 (prep_queries_kernel then only quantises; the oracle's distances with
    normalize_query=False is the same composition).  Dense queries then go through normalise + quantise unprepared.  The pool's
    own claims (every int8, exact ties of both signs, clipping, beyond +-A) are asserted on the host by i8_query_values()."""
    O = oracle
    A = QUANT_A
    orc, idx = int8_probe(O, hip, dim, A)
    vals = i8_query_values()
    B = vals.size
    Q = np.zeros((B, dim), np.float32)
    Q[:, dim - 1] = A
    Q[np.arange(B), np.arange(B) % (dim - 1)] = vals
    row_ids = np.arange(1, dim + 1, dtype=np.uint32)
    got = idx.distance_batch(Q, all_ids(B, dim), prepared=True)
    for b in range(B):
        want = orc.distances(Q[b], row_ids, normalize_query=False).astype(np.float32)
        assert np.array_equal(bits(got[b]), bits(want)), ("prepared", dim, b, vals[b])
    rng = np.random.default_rng(7 * dim)
    Qd = np.concatenate([np.resize(rng.permutation(vals), 33 * dim).reshape(33, dim), rng.standard_normal((17, dim)).astype(np.float32),
                         np.zeros((1, dim), np.float32)]).astype(np.float32)
    got = idx.distance_batch(Qd, all_ids(Qd.shape[0], dim))
    for b in range(Qd.shape[0]):
        want = orc.distances(Qd[b], row_ids).astype(np.float32)
        assert np.array_equal(bits(got[b]), bits(want)), ("normalised", dim, b)
    # AbsMax 0 (an untrained or all-zero quantizer): every query quantises to zeros, its norm 0 is replaced by 1, the dot product is 0
    # and the distance 1 - 0 / (1 * 127) = 1 for every row
    orc0, idx0 = int8_probe(O, hip, dim, 0.0)
    got = idx0.distance_batch(Qd, all_ids(Qd.shape[0], dim))
    for b in range(Qd.shape[0]):
        want = orc0.distances(Qd[b], row_ids)
        assert np.all(want == 1.0) and np.all(got[b] == np.float32(1.0)), ("AbsMax 0", dim, b)


# ---- 2. the distance tile ----------------------------------------------------------------------------------------------------------
def dev_form_on_a_stream(idx, Q, calls, what):
    """kdb_distance_batch_dev on a stream of the caller's (not the default one) gives the host form's bits"""
    import torch
    s = torch.cuda.Stream()
    for ids, host in calls:
        B = ids.shape[0]
        d_q = torch.from_numpy(Q[:B].copy()).cuda()
        d_ids = torch.from_numpy(ids.view(np.int32).copy()).cuda()
        d_out = torch.zeros(ids.shape, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        idx.distance_batch_dev(d_q, d_ids, d_out, stream=s.cuda_stream)
        s.synchronize()
        assert np.array_equal(bits(d_out.cpu().numpy()), bits(host)), (what, ids.shape)


@pytest.mark.gpu
@pytest.mark.parametrize("metric,prec", CELLS)
def test_distance_tile_at_the_chunk_boundary(oracle, hip, metric, prec):
    """distance_tile_kernel<prec, metric> at C around its 32-candidate chunk and at B 1 and 9: the oracle's values; +Inf for id 0 and
    ids that name no row; a deleted id keeps its value -- the reference's distFn (hnsw_index.go:2386-2458) reads the node's vector
    and never its Deleted flag, which searchLayerUnlocked tests only after the distance is computed (:2566, :2584); the _dev form on
    a stream of the caller's; KDB_SEARCH_PREPARED with the numpy-prepared query."""
    O = oracle
    n, dim = 200, 70
    orc, idx = build_pair(O, hip, make_corpus(n, dim, "normal", seed=21), metric, precision=prec, m=8, efc=40)
    orc.set_arith(O.ARITH_HIP_WAVE)
    cap = n + 8                                                                          # (build_pair's capacity)
    nowhere = np.array([0, n + 1, cap, 0xffffffff], np.uint32)
    rng = np.random.default_rng(100 * metric + prec)
    Q = rng.standard_normal((9, dim)).astype(np.float32)

    def check(got, Qb, ids):
        for b in range(ids.shape[0]):
            live = (ids[b] >= 1) & (ids[b] <= n)
            want = orc.distances(Qb[b], ids[b][live])
            if prec == I8:                                                               # the float rounding of the float64 distance
                assert np.array_equal(bits(got[b][live]), bits(want.astype(np.float32))), (metric, prec, ids.shape, b)
            else:
                assert np.array_equal(score(metric, prec, got[b][live]), want), (metric, prec, ids.shape, b)
            assert np.all(np.isposinf(got[b][~live])), (metric, prec, ids.shape, b, ids[b][~live], got[b][~live])

    calls = []
    for C in (1, 31, 32, 33, 70):
        for B in (1, 9):
            ids = rng.integers(1, n + 1, size=(B, C)).astype(np.uint32)
            if ids.size >= 8:
                ids.reshape(-1)[1:8:2] = nowhere
            got = idx.distance_batch(Q[:B], ids)
            check(got, Q[:B], ids)
            calls.append((ids, got))
    ids = nowhere[None, :].copy()
    got = idx.distance_batch(Q[:1], ids)
    assert np.all(np.isposinf(got))
    calls.append((ids, got))
    dev_form_on_a_stream(idx, Q, calls[-4:], (metric, prec))
    # the caller's own preparation
    if prec != I8:
        Qp = np.stack([np_prepared(q, metric, prec) for q in Q])
        for ids, host in calls:
            got = idx.distance_batch(Qp[:ids.shape[0]], ids, prepared=True)
            assert np.array_equal(bits(got), bits(host)), (metric, prec, ids.shape)
    # deleted rows keep their distance
    dead = np.unique([ids.ravel()[0] for ids, _ in calls[:-1]] + list(range(2, n + 1, 2))).astype(np.uint32)   # every call holds one
    idx.Delete(dead)
    for ids, before in calls:
        assert np.isin(ids, dead).any() or ids is calls[-1][0]
        got = idx.distance_batch(Q[:ids.shape[0]], ids)
        assert np.array_equal(bits(got), bits(before)), (metric, prec, ids.shape)


# ---- 3. one answer from both preparations ------------------------------------------------------------------------------------------
def section3_queries(metric, prec, dim):
    """(live [P, dim], names, dead [D, dim]): the pools of section 1 as far as they test the PREPARATION of this cell.  L2 leaves out
    the float32 queries of 1e18 and more: nothing is prepared there, and their squared differences absorb every row (all rows
    tie) or overflow.  dead: not finite once prepared."""
    f = np.float32
    rng = np.random.default_rng(17 * dim + 3 * metric + prec)
    pool = f32_query_pool(dim, seed=1)
    if metric == L2:
        for nm in ("overflow_sum_1e19", "overflow_sum_2e19", "mixed_magnitudes"):
            del pool[nm]
    if prec == F16:
        c = f16_edge_values()
        pool["f16_edges_dense"] = np.resize(rng.permutation(c), dim).astype(f)
        big = rng.standard_normal(dim).astype(f)
        big[[1, dim - 1]] = [65504, -65519.996]                                          # the largest half, reached from both sides
        pool["f16_largest"] = big
    if prec == I8:
        pool["i8_edges_dense"] = np.resize(rng.permutation(i8_query_values()), dim).astype(f)
    base = rng.standard_normal(dim).astype(f)
    dead = []
    for at, v in ((0, np.nan), (dim - 1, np.inf), (dim // 2, -np.inf)):
        q = base.copy()
        q[at] = v
        dead.append(q)
    if prec == F16:                                                                      # finite values, infinite halves
        for at, v in ((0, 65520.0), (dim - 1, -1e6), (dim // 2, 3e38)):
            q = base.copy()
            q[at] = v
            dead.append(q)
        dead.append(np.full(dim, 70000.0, f))
    names = list(pool)
    live = np.stack([pool[nm] for nm in names])
    dead = np.stack(dead).astype(f)
    assert all(np.isfinite(np_prepared(q, metric, prec)).all() for q in live)
    assert not any(np.isfinite(np_prepared(q, metric, prec)).all() for q in dead)
    return live, names, dead


def decoded_rows(orc, prec):
    """GetNodeData's vector for every stored row (hnsw_index.go:2909-2959), row 0 unused"""
    r = orc.rows()
    if prec == F32:
        return r
    if prec == F16:
        return r.view(np.float16).astype(np.float32)
    return (r.astype(np.float32) / np.float32(127.0)) * np.float32(orc.absmax)          # Dequantize (quantizer.go:181-198)


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [70, 768])
@pytest.mark.parametrize("metric,prec", CELLS)
def test_one_answer_from_walk_scan_by_id_and_distance_tile(oracle, hip, metric, prec, dim):
    O = oracle
    k, ef = 10, 64
    live, names, deadq = section3_queries(metric, prec, dim)
    P, D = live.shape[0], deadq.shape[0]
    n = 300
    # some live queries are stored too (the last ids): by-id calls search with them.  Not the ones whose stored form would be one
    # more (near-)zero row: two rows at one place make EVERY query a tied one
    stored = [p for p, nm in enumerate(names) if nm not in ("denormal_sum", "underflow_sum", "overflow_sum_1e19", "overflow_sum_2e19")]
    S = len(stored)
    X = np.concatenate([make_corpus(n - S, dim, "normal", seed=5), live[stored]])
    orc, idx = build_pair(O, hip, X, metric, precision=prec, m=8, efc=60)
    orc.set_arith(O.ARITH_HIP_WAVE)
    d64 = {"dist64": True} if prec == I8 else {}
    rows = np.arange(1, n + 1, dtype=np.uint32)

    def as_score(d):
        return np.asarray(d, dtype=np.float64) if prec == I8 else score(metric, prec, d)

    def as_tile(d):
        return np.asarray(d, dtype=np.float32)                                          # int8: the float rounding of the float64 answer

    # the oracle, once per query
    def expect(q):
        dall = orc.distances(q, rows)
        return dict(walk=orc.search(q, k, ef=ef), scan=orc.flat_scan(q, k), all=dall, tied=np.unique(dall).size < n)

    exp = [expect(q) for q in live]
    Qall = np.concatenate([live, deadq])
    tile = idx.distance_batch(Qall, all_ids(P + D, n))
    for p in range(P):
        want = exp[p]["all"]
        assert np.array_equal(bits(tile[p]), bits(want.astype(np.float32))) if prec == I8 else np.array_equal(as_score(tile[p]), want), (names[p],)
    assert np.all(np.isposinf(tile[P:])), "a query that is not finite once prepared is infinitely far from every row"

    def check(what, res, sel, want_key, ids_too, exp, tile, names):
        """res = (ids, dist, cnt) of the queries sel; an index of sel beyond exp's length is a dead query"""
        ids, dist, cnt = res
        for r, p in enumerate(sel):
            c = int(cnt[r]) & COUNT_MASK
            if p >= len(exp):
                assert c == 0 and not ids[r].any() and np.all(np.isposinf(dist[r])), (what, "dead query", p - len(exp), c, ids[r], dist[r])
                continue
            got_ids = ids[r, :c].astype(np.int64)
            assert np.all(got_ids >= 1) and np.all(got_ids <= n) and not ids[r, c:].any(), (what, names[p])
            assert np.array_equal(bits(as_tile(dist[r, :c])), bits(tile[p][got_ids - 1])), (what, names[p], "the tile reports another float for a pair")
            oi, od = exp[p][want_key]
            if ids_too(exp[p]["tied"]):
                assert c == len(oi) and np.array_equal(got_ids, oi), (what, names[p], got_ids, oi)
            if want_key == "scan" or ids_too(exp[p]["tied"]):
                assert c == len(od) and np.array_equal(as_score(dist[r, :c]), od), (what, names[p])

    never_tied, always = (lambda tied: not tied), (lambda tied: True)
    to = (exp, tile, names)
    for a in range(0, P + D, 3):                                                         # three queries: four waves per query
        sel = np.arange(a, min(a + 3, P + D))
        check("walk, 3 queries", idx.search_batch(Qall[sel], k, ef, **d64), sel, "walk", never_tied, *to)
    sel = np.arange(300) % (P + D)                                                       # 300 queries: one wave per query
    check("walk, 300 queries", idx.search_batch(Qall[sel], k, ef, **d64), sel, "walk", never_tied, *to)
    sel = np.arange(P + D)
    check("heap-order walk", idx.search_batch(Qall, k, ef, **d64, **HEAP), sel, "walk", always, *to)
    check("exact scan", idx.flat_scan_batch(Qall, k, **d64), sel, "scan", never_tied, *to)
    # a stored copy of a live query as the query: the reference searches with GetNodeData's vector, prepared again
    dec = decoded_rows(orc, prec)
    src = np.arange(n - S + 1, n + 1, dtype=np.uint32)
    to = ([expect(dec[i]) for i in src], idx.distance_batch(dec[src], all_ids(S, n)), [names[p] for p in stored])
    sel = np.arange(S)
    check("search_by_id", idx.search_by_id(src, k, ef, **d64), sel, "walk", never_tied, *to)
    check("search_by_id, heap order", idx.search_by_id(src, k, ef, **d64, **HEAP), sel, "walk", always, *to)
    check("flat_scan_by_id", idx.flat_scan_by_id(src, k, **d64), sel, "scan", never_tied, *to)
