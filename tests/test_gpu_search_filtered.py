"""A filtered request as one call (kdb_search_filtered): programs in, answers out.  2000 x 16 rows with an oracle graph (m 8, efC 20,
as test_cpp_host.py builds) in L2 / float32, L2 / float16 and cosine / int8.  Programs allowing about 50 % of the ids (walk), about
2 % (exact scan) and nothing (empty), plus queries without a filter, 64 queries interleaved across them.  Per query the answer --
ids, distance bits, count -- equals search_batch / flat_scan_batch on the same index with the bitset that tests/filter_ref.py (the
plain-Python FindIDsByFilter) makes from the same documents; out_route and out_card are as the routing rule says."""
import functools

import numpy as np
import pytest

import filter_ref as R

pytestmark = pytest.mark.gpu

L2, COSINE = 0, 1
F32, F16, I8 = 0, 1, 2
N, DIM = 2000, 16
SCHEMA = {"half": {"f64": 2, "code": None, "dict": {}}, "tag": {"f64": None, "code": 0, "dict": {"rare": 1, "common": 2}},
          "_is_historical": {"f64": None, "code": 5, "dict": {"true": 1, "false": 2}}}
FILTERS = ["half>=0.5 AND _is_historical!='true'",     # about half of the ids: the walk
           "tag='rare'",                               # about 2 %: the exact scan
           "tag='rare' AND half>2",                    # nothing: no results
           "tag!=rare"]                                # about 98 %: the walk


@functools.lru_cache(maxsize=None)
def setup(prec):
    from oracle import oracle as O
    import kektordb_amd as hip
    O.build()
    metric = COSINE if prec == I8 else L2
    rng = np.random.default_rng(7)
    X = rng.random((N, DIM), dtype=np.float32)
    if prec == F16:
        X = (X * 0.25).astype(np.float32)
    o = O.OracleIndex(DIM, metric, prec, 8, 20, seed=3)
    if prec == I8:
        o.set_absmax(float(np.abs(X).max()))
    o.add_many(X)
    idx = hip.HipIndex(DIM, metric, prec, 8, 20, capacity=N + 11)
    idx.upload_rows(o.rows()[1:], 1)
    if prec == I8:
        idx.upload_norms(o.norms()[1:], 1)
        idx.set_quantizer(o.absmax)
    idx.upload_graph_obj(o.export_graph())
    dead = set(rng.choice(np.arange(1, N + 1), N // 20, replace=False).tolist())
    idx.Delete(sorted(dead))
    half = rng.random(N + 1)
    tag = np.where(rng.random(N + 1) < 0.02, 1, 2).astype(np.uint32)
    hist = np.where(rng.random(N + 1) < 0.01, 1, 0).astype(np.uint32)       # 1 % marked historical, the others carry no value
    idx.set_column(2, 1, half[1:], 1)
    idx.set_column(0, 2, tag[1:], 1)
    idx.set_column(5, 2, hist[1:], 1)
    docs = {i: {"half": float(half[i]), "tag": "rare" if tag[i] == 1 else "common", **({"_is_historical": True} if hist[i] else {})}
            for i in range(1, N + 1)}
    db = R.MetaDB(docs, dead)
    words = (N >> 6) + 1
    sets = [db.find_ids(f) for f in FILTERS]
    Q = (X[rng.choice(N, 64, replace=False)] + 0.01 * rng.random((64, DIM), dtype=np.float32)).astype(np.float32)
    return idx, Q, sets, [R.bitset(s, words) for s in sets]


@pytest.mark.parametrize("prec", [F32, F16, I8])
def test_routes_and_parity(hip, prec):
    from kektordb_amd.index import compile_filter, NO_FILTER, ROUTE_WALK, ROUTE_SCAN, ROUTE_EMPTY
    idx, Q, sets, bits = setup(prec)
    live = N - N // 20
    assert 0.4 * live < len(sets[0]) < 0.6 * live and 0 < len(sets[1]) < 0.1 * N and not sets[2] and len(sets[3]) > 0.9 * live
    progs = [compile_filter(f, SCHEMA) for f in FILTERS]
    poq = np.array([[0, 1, 2, -1, 3][b % 5] for b in range(64)], dtype=np.int64)
    k, ef = 5, 40
    ids, dist, cnt, route, card = idx.search_filtered(Q, k, ef, progs, poq, flat_selectivity=0.1)
    assert card.tolist() == [len(s) for s in sets]
    want_route = {0: ROUTE_WALK, 1: ROUTE_SCAN, 2: ROUTE_EMPTY, 3: ROUTE_WALK, -1: ROUTE_WALK}
    assert route.tolist() == [want_route[int(p)] for p in poq]
    for p in (-1, 0, 1, 2, 3):
        sel = np.nonzero(poq == p)[0]
        if p == 2:                               # the empty program returns nothing -- not the unfiltered top-k of the exact scan
            assert not cnt[sel].any() and not ids[sel].any()
            wi, wd, wc = idx.flat_scan_batch(Q[sel], k, allow_bits=bits[2])     # the trap: an empty list means "no filter" there
            assert wc.all()
            continue
        if p == 1:
            wi, wd, wc = idx.flat_scan_batch(Q[sel], k, allow_bits=bits[1])
        else:
            wi, wd, wc = idx.search_batch(Q[sel], k, ef, allow_bits=None if p < 0 else bits[p])
        assert np.array_equal(cnt[sel], wc), (p, cnt[sel], wc)
        assert wc.any()
        for j, b in enumerate(sel):
            c = int(wc[j])
            assert np.array_equal(ids[b, :c], wi[j, :c]), (p, b, ids[b], wi[j])
            assert np.array_equal(dist[b, :c].view(np.uint32), wd[j, :c].view(np.uint32)), (p, b)
            assert p < 0 or all(int(i) in sets[p] for i in ids[b, :c])
    # every query on ONE program that scans; every query without a filter; P = 1
    for one, fn in ((1, lambda: idx.flat_scan_batch(Q, k, allow_bits=bits[1])), (-1, lambda: idx.search_batch(Q, k, ef))):
        ids, dist, cnt, route, card = idx.search_filtered(Q, k, ef, [progs[1]], np.full(64, 0 if one == 1 else -1), flat_selectivity=0.1)
        wi, wd, wc = fn()
        assert np.array_equal(cnt, wc) and route.tolist() == [ROUTE_SCAN if one == 1 else ROUTE_WALK] * 64
        for b in range(64):
            c = int(wc[b])
            assert np.array_equal(ids[b, :c], wi[b, :c]) and np.array_equal(dist[b, :c].view(np.uint32), wd[b, :c].view(np.uint32))
    # flat_selectivity 0: nothing takes the scan
    ids, dist, cnt, route, card = idx.search_filtered(Q[:8], k, ef, progs, np.full(8, 1), flat_selectivity=0.0)
    wi, wd, wc = idx.search_batch(Q[:8], k, ef, allow_bits=bits[1])
    assert route.tolist() == [ROUTE_WALK] * 8 and np.array_equal(cnt, wc)
    assert all(np.array_equal(ids[b, :int(wc[b])], wi[b, :int(wc[b])]) for b in range(8))


def test_large_k_stays_on_the_walk_or_takes_the_any_k_scan(hip):
    """k = 1025 with the 2 % program stays on the walk (the exact scan serves k <= 1024); k = 200 takes the scan, one list at a time"""
    from kektordb_amd.index import compile_filter, ROUTE_WALK, ROUTE_SCAN
    idx, Q, sets, bits = setup(F32)
    progs = [compile_filter(f, SCHEMA) for f in FILTERS]
    poq = np.array([1, 1, 0, 1], dtype=np.int64)
    ids, dist, cnt, route, card = idx.search_filtered(Q[:4], 1025, 1100, progs, poq, flat_selectivity=0.1)
    assert route.tolist() == [ROUTE_WALK] * 4
    for b in range(4):
        wi, wd, wc = idx.search_batch(Q[b:b + 1], 1025, 1100, allow_bits=bits[int(poq[b])])
        c = int(wc[0])
        assert int(cnt[b]) == c and c > 0 and np.array_equal(ids[b, :c], wi[0, :c]) and np.array_equal(dist[b, :c].view(np.uint32), wd[0, :c].view(np.uint32))
    ids, dist, cnt, route, card = idx.search_filtered(Q[:4], 200, 300, progs, poq, flat_selectivity=0.1)
    assert route.tolist() == [ROUTE_SCAN, ROUTE_SCAN, ROUTE_WALK, ROUTE_SCAN]
    for b in range(4):
        if poq[b] == 1:
            wi, wd, wc = idx.flat_scan_batch(Q[b:b + 1], 200, allow_bits=bits[1])
            assert int(wc[0]) == len(sets[1])
        else:
            wi, wd, wc = idx.search_batch(Q[b:b + 1], 200, 300, allow_bits=bits[0])
        c = int(wc[0])
        assert int(cnt[b]) == c and np.array_equal(ids[b, :c], wi[0, :c]) and np.array_equal(dist[b, :c].view(np.uint32), wd[0, :c].view(np.uint32))


def test_refusals(hip):
    from kektordb_amd.index import compile_filter
    idx, Q, sets, bits = setup(F32)
    progs = [compile_filter(FILTERS[0], SCHEMA)]
    with pytest.raises(hip.KdbError, match="status -1"):
        idx.search_filtered(Q[:2], 5, 40, progs, [0, 1])                    # program 1 does not exist
    with pytest.raises(hip.KdbError, match="status -1"):
        idx.search_filtered(Q[:2], 5, 40, progs, [0, 0], flat_selectivity=1.5)
    with pytest.raises(hip.KdbError, match="status -1"):
        idx.search_filtered(Q[:2], 0, 40, progs, [0, 0])
    bad = progs[0].copy()
    bad["flags"][-1] = 0                                                     # the final END_BLOCK is missing
    with pytest.raises(hip.KdbError, match="status -1"):
        idx.search_filtered(Q[:2], 5, 40, [bad], [0, 0])
    ids, dist, cnt, route, card = idx.search_filtered(Q[:2], 5, 40, progs, [0, -1])   # ... and the index still answers
    assert cnt.all()
