"""Search by stored id (kdb_index_decode_rows, kdb_search_by_id[_dev], kdb_flat_scan_by_id[_dev]; by_id.hip).

The feature is a composition: query b of a by-id call is the decoded row of ids[b] (GetNodeData, hnsw_index.go:2909-2959) and the
answer is that of the existing entry point for that float32 vector.  So the bars are equalities:
  1. decode = the host's decode of the downloaded rows, bit for bit (int8: the oracle's orc_dequantize);
  2. every by-id entry point = search_batch / flat_scan_batch on those vectors: ids, distance bits, counts, per-query trace arrays and
     the call's counters.  A source that is not found must get nothing and must not be walked: in the reference call its vector is
     a NaN row, which the library answers with count 0 and no walk (kektor_hip.h, "Conventions"), so the counters have to agree too.
     The exact scan has no such rule; there the reference call scans the decoded zero row (the same device work) and the rows of the
     not-found sources are checked against "count 0, zero ids" instead;
  3. = the oracle's search of the decoded vector under ARITH_HIP_WAVE, ids, distance bits and per-query counters: the 203-id lists
     with n_tied == 0, every id in one call under KDB_SEARCH_HEAP_ORDER (float32 distances collide somewhere among thousands of walks);
  4. not-found sources; 5. KDB_BY_ID_DROP_SELF = the host-side composition of the k + 1 call; 6. concurrent callers, and a writer
     against the calls that take turns on the index's staging buffer.

Graphs come from OracleIndex.add (tests/test_gpu_refine.py's Case: m = 8, efC = 40, unique rows), built once per process."""
import functools
import threading

import numpy as np
import pytest

from test_gpu_refine import Case

pytestmark = pytest.mark.gpu

L2, COSINE = 0, 1
F32, F16, I8 = 0, 1, 2
NOPE = 0xffffffff
CASES = ["A", "B", "C", "D", "E"]
# seed of each case's 203-id list, chosen so that no walk of the batches compared with the oracle's plain walk meets two nodes at
# equal distance (n_tied == 0 is asserted there)
LIST_SEED = {"A": 101, "B": 99, "C": 99, "D": 99, "E": 103}


class Setup:
    """one case: the oracle side (Case), the device index, the host decode of every row, the id lists"""

    def __init__(self, name):
        from oracle import oracle as O
        import kektordb_amd as hip
        O.build()
        mk = {
            "A": lambda: Case(O, COSINE, F32, 3000, 100, 8, 40, seed=21, deleted_frac=0.05, delete_entry=True),
            "B": lambda: Case(O, L2, F32, 3000, 64, 8, 40, seed=22, deleted_frac=0.05),
            "C": lambda: Case(O, L2, F16, 3000, 72, 8, 40, seed=23, deleted_frac=0.05),
            "D": lambda: Case(O, COSINE, I8, 3000, 100, 8, 40, seed=24, deleted_frac=0.05),
            "E": lambda: Case(O, COSINE, F32, 4096, 768, 8, 40, seed=25, deleted_frac=0.05),
        }
        c = self.case = mk[name]()
        self.name, self.O, self.n, self.dim, self.prec = name, O, c.count, c.dim, c.prec
        idx = self.idx = hip.HipIndex(c.dim, c.metric, c.prec, c.m, c.ef, capacity=c.count + 8)
        idx.upload_rows(c.rows[1:], 1)
        if c.prec == I8:
            idx.upload_norms(c.norms[1:], 1)
            idx.set_quantizer(c.orc.absmax)
        idx.upload_graph_obj(c.g)
        # the host's decode (assertion 1): row 0 stays zero
        rows = idx.download_rows(1, c.count)
        assert np.array_equal(rows.view(np.uint8), c.rows[1:].view(np.uint8))
        wide = np.zeros((c.count + 1, c.dim), dtype=np.float32)
        if c.prec == F32:
            wide[1:] = rows
        elif c.prec == F16:
            wide[1:] = rows.view(np.float16).astype(np.float32)
        else:
            r8 = np.ascontiguousarray(rows, dtype=np.int8)
            out = np.zeros(r8.shape, dtype=np.float32)
            O.lib().orc_dequantize(r8.ctypes.data, r8.size, np.float32(c.orc.absmax), out.ctypes.data)
            wide[1:] = out
        self.wide = wide
        self.dead = np.nonzero(c.deleted)[0].astype(np.uint32)
        self.live = np.nonzero(~c.deleted[1:])[0].astype(np.uint32) + 1
        assert len(self.dead) == int(c.count * 0.05)
        assert bool(c.deleted[c.g.entry]) == (name == "A")       # case A: the entry point is among the deleted ids
        self.even = np.zeros((c.count >> 6) + 1, dtype=np.uint64)
        for i in range(2, c.count + 1, 2):
            self.even[i >> 6] |= np.uint64(1) << np.uint64(i & 63)
        self.make_lists(LIST_SEED[name])
        self._orc = {}

    def make_lists(self, seed):
        """the id lists: each multi-id list holds deleted ids, 0, count+1, 0xffffffff, a repeated id and the entry point"""
        c = self.case
        rng = np.random.default_rng(seed)
        special = [int(self.dead[0]), int(self.dead[1]), 0, c.count + 1, NOPE, int(c.g.entry)]
        pick = rng.choice(self.live, 196, replace=False).tolist()
        mid = np.array(pick + [pick[5]] + special, dtype=np.uint32)
        rng.shuffle(mid)
        assert mid.size == 203
        every = np.array(list(range(1, c.count + 1)) + [pick[5]] + special, dtype=np.uint32)
        self.lists = {"mid": mid, "all": every}
        self.singles = [np.array([v], dtype=np.uint32) for v in [pick[0]] + special]   # B = 1, one call each

    def found(self, ids):
        ids = np.asarray(ids, dtype=np.int64)
        ok = (ids >= 1) & (ids <= self.n)
        ok[ok] = ~self.case.deleted[ids[ok]]
        return ok

    def vectors(self, ids, miss=0.0):
        """the decoded vectors of `ids` on the host; not-found rows are `miss`"""
        ok = self.found(ids)
        v = np.full((len(ids), self.dim), miss, dtype=np.float32)
        v[ok] = self.wide[np.asarray(ids, dtype=np.int64)[ok]]
        return v, ok

    def oracle_search(self, id_, k, ef, allow):
        key = (int(id_), k, ef, allow is not None)
        if key not in self._orc:
            self._orc[key] = self.case.orc.search(self.wide[int(id_)], k, allow=allow, ef=ef, counters=True)
        return self._orc[key]


@functools.lru_cache(maxsize=None)
def setup(name):
    return Setup(name)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def dev_call(S, fn, ids, k, ef, allow, dist64=False, drop_self=False, trace=False):
    """a *_dev entry point with torch tensors; -> (ids, dist, count[, (n_dist, n_hops)]) on the host"""
    import torch
    import ctypes as C
    idx = S.idx
    B = len(ids)
    d_ids = torch.from_numpy(np.ascontiguousarray(ids).view(np.int32)).cuda()
    oi = torch.full((B, k), -1, dtype=torch.int32, device="cuda")
    od = torch.full((B, k), -7.0, dtype=torch.float64 if dist64 else torch.float32, device="cuda")
    oc = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    d_al = None if allow is None else torch.from_numpy(allow.view(np.int64)).cuda()
    nd = nh = None
    if trace:
        nd = torch.full((B,), -1, dtype=torch.int32, device="cuda")
        nh = torch.full((B,), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        idx.L.kdb_search_set_trace(idx.h, C.c_void_p(nd.data_ptr()), C.c_void_p(nh.data_ptr()), 1)
    try:
        if fn == "walk":
            idx.search_by_id_dev(d_ids, k, ef, oi, od, oc, d_al, dist64=dist64, drop_self=drop_self)
        else:
            idx.flat_scan_by_id_dev(d_ids, k, oi, od, oc, d_al, dist64=dist64, drop_self=drop_self)
        idx.sync()
    finally:
        if trace:
            idx.L.kdb_search_set_trace(idx.h, None, None, 0)
    out = (oi.cpu().numpy().view(np.uint32), od.cpu().numpy(), oc.cpu().numpy().view(np.uint32))
    if trace:
        return out + ((nd.cpu().numpy().view(np.uint32), nh.cpu().numpy().view(np.uint32)),)
    return out


def ctr(idx):
    c = idx.counters()
    return c["n_dist"], c["n_hops"], c["n_tied"], c["n_dropped"]


# ---- 1. decode ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_decode_rows_equals_the_host_decode(name):
    import torch
    S = setup(name)
    for ids in S.singles + [S.lists["mid"], S.lists["all"]]:
        want, ok = S.vectors(ids)
        got, found = S.idx.decode_rows(ids)
        assert same(got, want), (name, len(ids))
        assert np.array_equal(found, ok)
        assert not got[~ok].any()                                # not-found rows are zero
        d_out = torch.full((len(ids), S.dim), float("nan"), device="cuda")
        d_found = torch.full((len(ids),), 9, dtype=torch.uint8, device="cuda")
        S.idx.decode_rows_dev(torch.from_numpy(ids.view(np.int32)).cuda(), d_out, d_found)
        S.idx.sync()
        assert same(d_out.cpu().numpy(), want) and np.array_equal(d_found.cpu().numpy().astype(bool), ok)
    e_dead = 1 if name == "A" else 0                             # (the "all" list: every id + a repeated live one + the specials)
    assert ok.sum() == len(S.live) + 2 - e_dead and (~ok).sum() == len(S.dead) + 5 + e_dead
    if S.prec == I8:                                             # an untrained quantizer dequantizes to zeros (quantizer.go:185-187)
        S.idx.set_quantizer(0.0)
        try:
            got, found = S.idx.decode_rows(S.lists["mid"])
        finally:
            S.idx.set_quantizer(S.case.orc.absmax)
        assert not got.any() and np.array_equal(found, S.found(S.lists["mid"]))
    out, found = S.idx.decode_rows(np.zeros(0, dtype=np.uint32))
    assert out.shape == (0, S.dim)


# ---- 2. by-id against the existing entry points on the decoded vectors -----------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_search_by_id_equals_search_batch_on_the_decoded_vectors(name):
    S = setup(name)
    idx = S.idx
    n_calls = 0
    for ids in S.singles + [S.lists["mid"], S.lists["all"]]:
        vq, ok = S.vectors(ids, miss=np.nan)
        for allow in (None, S.even):
            for ef in (12, 50):
                for k in (1, 10):
                    for d64 in ((False, True) if S.prec == I8 else (False,)):
                        if len(ids) == 1 and (k, ef) != (10, 50) and ok[0]:
                            continue                              # (the B = 1 lists: one shape for the found source, all for the others)
                        wi, wd, wc, (wnd, wnh) = idx.search_batch(vq, k, ef, allow, trace=True, dist64=d64)
                        want_ctr = ctr(idx)
                        assert not wc[~ok].any() and not wi[~ok].any()    # the guarantee the feature leans on
                        gi, gd, gc, (gnd, gnh) = idx.search_by_id(ids, k, ef, allow, trace=True, dist64=d64)
                        assert ctr(idx) == want_ctr, (name, len(ids), k, ef, d64)
                        assert same(gi, wi) and same(gd, wd) and same(gc, wc), (name, "host", len(ids), k, ef, allow is not None, d64)
                        assert same(gnd, wnd) and same(gnh, wnh)
                        di, dd, dc, (dnd, dnh) = dev_call(S, "walk", ids, k, ef, allow, dist64=d64, trace=True)
                        assert ctr(idx) == want_ctr
                        assert same(di, wi) and same(dd, wd) and same(dc, wc), (name, "dev", len(ids), k, ef, allow is not None, d64)
                        assert same(dnd, wnd) and same(dnh, wnh)
                        if ok.any() and allow is None:
                            assert gc[ok].min() >= 1
                        n_calls += 1
    assert n_calls >= 16


@pytest.mark.parametrize("name", CASES)
def test_flat_scan_by_id_equals_flat_scan_batch_on_the_decoded_vectors(name):
    S = setup(name)
    idx = S.idx
    for ids in S.singles + [S.lists["mid"], S.lists["all"]]:
        vq, ok = S.vectors(ids)
        for allow in (None, S.even):
            for k in (1, 10):
                for d64 in ((False, True) if S.prec == I8 else (False,)):
                    wi, wd, wc = idx.flat_scan_batch(vq, k, allow, dist64=d64)
                    want_ctr = ctr(idx)[:2]
                    for form in ("host", "dev"):
                        if form == "host":
                            gi, gd, gc = idx.flat_scan_by_id(ids, k, allow, dist64=d64)
                        else:
                            gi, gd, gc = dev_call(S, "flat", ids, k, 0, allow, dist64=d64)
                        assert ctr(idx)[:2] == want_ctr
                        assert same(gi[ok], wi[ok]) and same(gd[ok], wd[ok]) and same(gc[ok], wc[ok]), (name, form, len(ids), k, allow is not None, d64)
                        assert not gc[~ok].any() and not gi[~ok].any() and np.isinf(gd[~ok]).all()
                        if ok.any():
                            assert gc[ok].min() == k
    if S.prec == F32 and name != "E":                            # k above 128: the any-k scan behind the same composition
        ids = S.lists["mid"]
        vq, ok = S.vectors(ids)
        wi, wd, wc = idx.flat_scan_batch(vq, 200)
        gi, gd, gc = idx.flat_scan_by_id(ids, 200)
        assert same(gi[ok], wi[ok]) and same(gd[ok], wd[ok]) and same(gc[ok], wc[ok]) and not gc[~ok].any()


# ---- 3. against the oracle ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_search_by_id_equals_the_oracle(name):
    S = setup(name)
    idx, c = S.idx, S.case
    k = 10
    # The 203-id lists: the library's plain walk against the oracle's, with n_tied == 0 asserted (LIST_SEED).  Every id in one call:
    # among thousands of walks a few meet two float32 distances that collide (7 of 3000 in case A, 48 of 4096 in case E -- no seed
    # avoids that), so that batch runs with KDB_SEARCH_HEAP_ORDER, under which a tied walk is the reference's as well: every found
    # id is compared, none is excluded.
    plans = [("mid", 12, None, False), ("mid", 50, None, False), ("mid", 50, S.even, False), ("all", 50, None, True)]
    for which, ef, allow, heap in plans:
        ids = S.lists[which]
        ok = S.found(ids)
        gi, gd, gc, (nd, nh) = idx.search_by_id(ids, k, ef, allow, trace=True, dist64=(S.prec == I8), heap_order=heap)
        print(f"case {name} list {which} ef {ef} allow {allow is not None} heap_order {heap}: {idx.counters()}")
        if not heap:
            assert idx.counters()["n_tied"] == 0, (name, which, ef)
        assert idx.counters()["n_dropped"] == 0
        for b in np.nonzero(ok)[0]:
            oi, od, (ond, onh) = S.oracle_search(ids[b], k, ef, allow)
            cb = int(gc[b])
            assert np.array_equal(gi[b, :cb], oi), (name, which, ef, int(ids[b]), gi[b, :cb], oi)
            got = gd[b, :cb].astype(np.float64)
            if S.prec == F32 and c.metric == COSINE:
                got = 1.0 - got
            assert np.array_equal(got, od), (name, which, ef, int(ids[b]))
            assert (int(nd[b]), int(nh[b])) == (ond, onh), (name, which, ef, int(ids[b]))
        assert not gc[~ok].any()


# ---- 4. sources that are not found -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "D"])
def test_sources_that_are_not_found(name):
    S = setup(name)
    idx = S.idx
    ids = np.array([0, S.n + 1, NOPE, int(S.dead[0]), int(S.dead[3]), 0, 1 << 30, S.n + 8], dtype=np.uint32)
    assert not S.found(ids).any()
    for allow in (None, S.even):
        for call in (lambda: idx.search_by_id(ids, 10, 50, allow), lambda: dev_call(S, "walk", ids, 10, 50, allow),
                     lambda: idx.search_by_id(ids, 10, 50, allow, drop_self=True), lambda: dev_call(S, "walk", ids, 10, 50, allow, drop_self=True),
                     lambda: idx.flat_scan_by_id(ids, 10, allow), lambda: dev_call(S, "flat", ids, 10, 0, allow),
                     lambda: idx.flat_scan_by_id(ids, 10, allow, drop_self=True), lambda: dev_call(S, "flat", ids, 10, 0, allow, drop_self=True)):
            gi, gd, gc = call()                                  # KDB_OK (no KdbError)
            assert not gc.any() and not gi.any()
    idx.search_by_id(ids, 10, 50)
    assert ctr(idx)[:2] == (0, 0)                                # nothing was walked
    # among found ones: the others are answered as alone
    mixed = np.array([0, int(S.live[10]), int(S.dead[0]), int(S.live[11]), NOPE], dtype=np.uint32)
    gi, gd, gc = idx.search_by_id(mixed, 10, 50)
    ai, ad, ac = idx.search_by_id(mixed[[1, 3]], 10, 50)
    assert same(gi[[1, 3]], ai) and same(gd[[1, 3]], ad) and same(gc[[1, 3]], ac) and not gc[[0, 2, 4]].any() and not gi[[0, 2, 4]].any()


# ---- 5. KDB_BY_ID_DROP_SELF ----------------------------------------------------------------------------------------------------------
def compose_drop_self(src, ids1, d1, c1, k):
    """the documented composition on the host: from the k + 1 answer, the entry whose id is the source's leaves; otherwise the last
    one when all k + 1 came back; entries behind the count are (0, +Inf)"""
    B = len(src)
    oi = np.zeros((B, k), dtype=np.uint32)
    od = np.full((B, k), np.inf, dtype=d1.dtype)
    oc = np.zeros(B, dtype=np.uint32)
    for b in range(B):
        c = int(c1[b])
        keep = [j for j in range(c) if int(ids1[b, j]) != int(src[b])]
        assert len(keep) >= c - 1                                # there is at most one
        keep = keep[:k]
        oi[b, :len(keep)] = ids1[b, keep]
        od[b, :len(keep)] = d1[b, keep]
        oc[b] = len(keep)
    return oi, od, oc


@pytest.mark.parametrize("name", ["A", "B", "C", "D"])
def test_drop_self_equals_the_host_side_composition(name, hip):
    S = setup(name)
    idx = S.idx
    d64 = S.prec == I8
    ids = S.lists["mid"]
    ok = S.found(ids)
    odd_live = [b for b in np.nonzero(ok)[0] if ids[b] % 2 == 1]
    assert odd_live
    for k in (1, 10):
        for allow in (None, S.even):
            for fn in ("walk", "flat"):
                if fn == "walk":
                    i1, d1, c1 = idx.search_by_id(ids, k + 1, 50, allow, dist64=d64)
                    gi, gd, gc = idx.search_by_id(ids, k, 50, allow, dist64=d64, drop_self=True)
                else:
                    i1, d1, c1 = idx.flat_scan_by_id(ids, k + 1, allow, dist64=d64)
                    gi, gd, gc = idx.flat_scan_by_id(ids, k, allow, dist64=d64, drop_self=True)
                wi, wd, wc = compose_drop_self(ids, i1, d1, c1, k)
                assert same(gi, wi) and same(gd, wd) and same(gc, wc), (name, fn, k, allow is not None)
                di, dd, dc = dev_call(S, fn, ids, k, 50, allow, dist64=d64, drop_self=True)
                assert same(di, wi) and same(dd, wd) and same(dc, wc), (name, fn, k, allow is not None, "dev")
                assert not (gi[ok] == ids[ok, None]).any()       # self is absent
                if allow is None and fn == "flat":
                    assert (i1[ok, 0] == ids[ok]).all()          # ... and was there: the exact scan ranks a stored row first
                if allow is not None:                            # an odd source under the even-id list: its own id is not among its k + 1
                    for b in odd_live:
                        assert int(ids[b]) not in i1[b].tolist() and int(c1[b]) == k + 1 and int(gc[b]) == k
                        assert same(gi[b], i1[b, :k])
    # k + 1 over the limit, and PREPARED: KDB_ERR_INVALID
    with pytest.raises(hip.KdbError, match=r"status -1"):
        idx.flat_scan_by_id(ids, 1024, drop_self=True)
    gi, gd, gc = idx.flat_scan_by_id(ids[:3], 1023, drop_self=True)     # the limit itself is served
    assert gi.shape == (3, 1023)
    for call in (lambda: idx.search_by_id(ids, 10, 50, flags=2), lambda: idx.flat_scan_by_id(ids, 10, flags=2)):
        with pytest.raises(hip.KdbError, match=r"status -1"):
            call()


# ---- 6. concurrency smoke ------------------------------------------------------------------------------------------------------------
def test_concurrent_by_id_and_query_callers_on_one_handle():
    S = setup("B")
    idx = S.idx
    k, ef, calls = 5, 30, 300
    rng = np.random.default_rng(3)
    id_sets = [np.append(rng.choice(S.live, 7, replace=False), S.dead[t]).astype(np.uint32) for t in range(8)]
    q_sets = [S.wide[rng.choice(S.live, 3, replace=False)] + np.float32(0.01) for _ in range(8)]
    want_id = [idx.search_by_id(s, k, ef) for s in id_sets]
    want_q = [idx.search_batch(q, k, ef) for q in q_sets]
    bad = []

    def by_id(t):
        for it in range(calls):
            j = (t + it) % 8
            got = idx.search_by_id(id_sets[j], k, ef)
            if not all(same(a, b) for a, b in zip(got, want_id[j])):
                bad.append(("by_id", t, it))

    def by_query(t):
        for it in range(calls):
            j = (t + it) % 8
            got = idx.search_batch(q_sets[j], k, ef)
            if not all(same(a, b) for a, b in zip(got, want_q[j])):
                bad.append(("query", t, it))

    th = [threading.Thread(target=by_id, args=(t,)) for t in range(4)] + [threading.Thread(target=by_query, args=(t,)) for t in range(4)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not bad, bad[:5]


def test_writers_against_the_calls_that_take_turns_on_the_staging_buffer():
    """four readers x 200 rounds of distance_batch, decode_rows, consensus and flat_scan_by_id (each takes a turn on the index's
    staging buffer) while a writer alternates mark_deleted and upload_norms: every answer is the one computed before the threads
    started, bit for bit, and nobody is left waiting.  The writer's ids are deleted already and it uploads the norms they have, so
    the index of the other tests stays as it was; the readers' ids are live ones."""
    S = setup("D")
    idx, c = S.idx, S.case
    rng = np.random.default_rng(12)
    mine = rng.choice(S.live, 24, replace=False).astype(np.uint32)
    theirs = S.dead[:6]
    Q = (S.wide[mine[:3]] + np.float32(0.01)).astype(np.float32)
    calls = [lambda: (idx.distance_batch(Q, mine.reshape(3, 8)),),
             lambda: idx.decode_rows(mine),
             lambda: tuple(v for v in idx.consensus(mine.reshape(3, 8), None, Q, None, want_centroid=True).values() if v is not None),
             lambda: idx.flat_scan_by_id(mine[:8], 5)]
    want = [call() for call in calls]
    assert S.idx.decode_rows(mine)[1].all() and not S.found(theirs).any()
    bad, stop = [], threading.Event()

    def reader(t):
        try:
            for it in range(200):
                for j in range(len(calls)):
                    if not all(same(a, b) for a, b in zip(calls[j](), want[j])):
                        bad.append(("reader", t, it, j))
        except Exception as e:                                  # (a thread's exception must fail the test, not vanish)
            bad.append(("reader", t, repr(e)))

    def writer():
        try:
            it = 0
            while not stop.is_set():
                d = int(theirs[it % len(theirs)])
                if it & 1:
                    idx.upload_norms(c.norms[d:d + 1], d)
                else:
                    idx.Delete(theirs[it % 3:it % 3 + 3].tolist())
                it += 1
        except Exception as e:
            bad.append(("writer", repr(e)))

    rd = [threading.Thread(target=reader, args=(t,), daemon=True) for t in range(4)]
    wr = threading.Thread(target=writer, daemon=True)
    wr.start()
    for t in rd:
        t.start()
    for t in rd:
        t.join(60)
    stop.set()
    wr.join(60)
    assert not any(t.is_alive() for t in rd + [wr])
    assert not bad, bad[:5]
    assert all(all(same(a, b) for a, b in zip(calls[j](), want[j])) for j in range(len(calls)))   # and serially afterwards


def test_vsearchsimilar_is_searchwithscores_per_id():
    S = setup("D")
    idx = S.idx
    ids = S.lists["mid"][:40]
    vq, ok = S.vectors(ids)
    got = idx.VSearchSimilar(ids, 10, efSearch=50)
    for b in range(len(ids)):
        want = idx.SearchWithScores(vq[b], 10, efSearch=50) if ok[b] else []
        assert got[b] == want
    drop = idx.VSearchSimilar(ids, 10, efSearch=50, dropSelf=True)
    assert all(int(ids[b]) not in [r.DocID for r in drop[b]] for b in range(len(ids)))
