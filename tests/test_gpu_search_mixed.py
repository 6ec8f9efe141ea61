"""Mixed search batches: every query its own k and efSearch, one launch (kdb_search_batch_mixed[_dev], kdb_mixed_plan.h).

A query's answer does not depend on which beam class walks it, as long as the class is large enough (test_gpu_walk_instantiations.py
shows every cell equal to the oracle); here a launch sized for the LARGEST effective ef of its batch walks all of them, and every
query -- not a sample -- is compared with the oracle's walk for its own (k, ef): ids, distance bits, count, n_dist, n_hops.

The pairs are those of test_gpu_walk_instantiations.py (2000 clustered rows, 30 copies of one row, every 13th id deleted, the oracle's
graph at efConstruction 20, ARITH_HIP_WAVE), one per module; the oracle's and the homogeneous answers are computed once per (query,
key) and left unchanged."""
import functools

import numpy as np
import pytest

from test_gpu_walk_instantiations import NQ, Pair

pytestmark = pytest.mark.gpu

F32, F16, I8 = 0, 1, 2
L2, COS = 0, 1

# (k, efSearch) of the requests.  Written down, not computed from the code under test; effective ef = max(ef, k).
KEYS = [(1, 1), (10, 0), (10, 16), (5, 64), (10, 65), (64, 100), (10, 128), (100, 129), (100, 100), (10, 200), (10, 256), (10, 257),
        (10, 300), (10, 1200)]
# launch class (the largest effective ef of the batch) -> (the keys that fit it, BS its launches must report: 1 / 2 / 4 register slots,
# 0 = the LDS beam)
CLASSES = {
    64: (KEYS[:4], 1),
    128: (KEYS[:7] + [(100, 100)], 2),
    256: (KEYS[:11], 4),
    300: (KEYS[:13], 0),
    1200: (KEYS, 0),
}
# (name) -> (precision, metric, dim, walk planes, NCH its walks report)
PAIRS = {
    "f32_cos_768_planes": (F32, COS, 768, True, 12),
    "f32_cos_768": (F32, COS, 768, False, 12),
    "f32_l2_640": (F32, L2, 640, True, 0),
    "f16_l2_96": (F16, L2, 96, True, 0),
    "i8_cos_96": (I8, COS, 96, True, 0),
}


class MixedPair:
    def __init__(self, name):
        prec, metric, dim, planes, self.nch = PAIRS[name]
        self.name = name
        self.p = Pair(prec, metric, dim, planes)
        self.kw = {"dist64": True} if prec == I8 else {}
        self._oracle, self._homog = {}, {}

    def oracle(self, qi, k, ef, allow=None, allow_key=None):
        """the oracle's answer for stored query qi at (k, ef): computed once, left unchanged"""
        key = (qi, k, ef, allow_key)
        if key not in self._oracle:
            self._oracle[key] = self.p.orc.search(self.p.Q[qi], k, allow=allow, ef=ef, counters=True)
        return self._oracle[key]

    def homogeneous(self, k, ef):
        """search_batch(Q, k, ef) with the tie flag, no heap-order pass: the fast walk's own answer for the twelve queries"""
        if (k, ef) not in self._homog:
            self._homog[(k, ef)] = self.p.idx.search_batch(self.p.Q, k, ef, trace=True, tie_flag=True, **self.kw)
        return self._homog[(k, ef)]


@functools.lru_cache(maxsize=None)
def _mp(name):
    return MixedPair(name)


def _batch(keys, B):
    """query b: stored query b % NQ with key (b + b // NQ) % len(keys) -- every key meets every query as B grows"""
    qi = np.arange(B) % NQ
    ki = (np.arange(B) + np.arange(B) // NQ) % len(keys)
    ks = np.array([keys[i][0] for i in ki], dtype=np.uint32)
    efs = np.array([keys[i][1] for i in ki], dtype=np.uint32)
    return qi, ks, efs


def _check_padding(ids, dist, cnt, stride):
    c = (cnt & 0x3fffffff).astype(np.int64)
    pad = np.arange(stride)[None, :] >= c[:, None]
    assert np.all(ids[pad] == 0) and np.all(np.isposinf(dist[pad]))


def _check_parity(mp, ef_max, B):
    p, hip = mp.p, mp.p.hip
    keys, bs = CLASSES[ef_max]
    qi, ks, efs = _batch(keys, B)
    Q = p.Q[qi]
    stride = int(ks.max())
    # under KDB_SEARCH_HEAP_ORDER: the oracle's answer for every query, ties included
    ids, dist, cnt, (nd, nh) = p.idx.search_batch_mixed(Q, ks, efs, trace=True, tie_flag=True, heap_order=True, **mp.kw)
    s = p.idx.launch_shape()[0]
    print(f"shape {mp.name} ef_max={ef_max} B={B}: {s}")
    assert (s["search"], s["B"], s["prec"], s["metric"], s["nch"]) == (1, B, p.prec, p.metric, mp.nch), s
    assert s["bs"] == bs and s["heap_pass"] == 1, (ef_max, s)      # the class of the launch, not of the smallest ef
    if B > 2000:
        assert s["waves"] == 1, s
        assert s["planes"] == int(mp.name == "f32_cos_768_planes" and bs != 0), s
    else:
        assert s["waves"] == 4, s                                   # latency mode
    assert ids.shape == (B, stride) and not np.any(cnt >> 30), (ef_max, B)
    _check_padding(ids, dist, cnt, stride)
    for b in range(B):
        k, ef = int(ks[b]), int(efs[b])
        oi, od, (ond, onh) = mp.oracle(int(qi[b]), k, ef)
        c = int(cnt[b])
        where = (mp.name, ef_max, B, b, k, ef)
        assert c == len(oi) <= k and np.array_equal(ids[b, :c], oi), (where, ids[b, :c], oi)
        assert np.array_equal(p.scores(dist[b, :c]), od), where
        assert (int(nd[b]), int(nh[b])) == (ond, onh), (where, int(nd[b]), int(nh[b]), ond, onh)
    # the fast walk's own answer: what the homogeneous search_batch(q, k, ef) returns, wherever that one saw no tie -- and a tie it saw
    # is seen here too
    ids, dist, cnt, (nd, nh) = p.idx.search_batch_mixed(Q, ks, efs, trace=True, tie_flag=True, **mp.kw)
    s1 = p.idx.launch_shape()[0]
    assert s1["heap_pass"] == 0 and all(s1[f] == s[f] for f in ("search", "prec", "metric", "nch", "bs", "waves", "planes", "B")), (s1, s)
    _check_padding(ids, dist, cnt, stride)
    n_clear = 0
    for b in range(B):
        k, ef = int(ks[b]), int(efs[b])
        hi, hd, hc, (hnd, hnh) = mp.homogeneous(k, ef)
        q = int(qi[b])
        where = (mp.name, ef_max, B, b, k, ef, "plain walk")
        if int(hc[q]) & hip.index.COUNT_TIED:
            assert int(cnt[b]) & hip.index.COUNT_TIED, where
            continue
        n_clear += 1
        c = int(hc[q])
        assert int(cnt[b]) == c, (where, int(cnt[b]), c)
        assert np.array_equal(ids[b, :c], hi[q, :c]), where
        assert np.array_equal(dist[b, :c].view(np.uint8), hd[q, :c].view(np.uint8)), where      # the bits
        assert (int(nd[b]), int(nh[b])) == (int(hnd[q]), int(hnh[q])), where
    assert n_clear > 0, (mp.name, ef_max, B)


@pytest.mark.parametrize("ef_max", list(CLASSES))
@pytest.mark.parametrize("name", list(PAIRS))
def test_mixed_parity_per_query_latency_mode(name, ef_max):
    _check_parity(_mp(name), ef_max, 48)


@pytest.mark.parametrize("ef_max", [64, 300])
@pytest.mark.parametrize("name", ["f32_cos_768_planes", "f32_cos_768"])
def test_mixed_parity_per_query_one_wave_per_query(name, ef_max):
    _check_parity(_mp(name), ef_max, 2400)


def _six_lists(n):
    """the lists of test_search_heterogeneous_allow_lists: 50 %, 20 %, 5 %, empty, three ids, id 0 only"""
    from kektordb_amd.index import dense_bitset
    rng = np.random.default_rng(5)
    words = (n >> 6) + 1
    lists = []
    for sel in (0.5, 0.2, 0.05):
        a = np.nonzero(rng.random(n + 1) < sel)[0]
        lists.append(dense_bitset(a[a >= 1], n))
    lists.append(np.zeros(words, np.uint64))
    lists.append(dense_bitset(np.array([1, 2, 3], np.uint64), n))
    only_zero = np.zeros(words, np.uint64)
    only_zero[0] = 1
    lists.append(only_zero)
    return np.stack(lists)


def _dev_call(mp, Q, ks, efs, stride, ef_max, lists=None, of_q=None, **flags):
    import torch
    dev = torch.device("cuda:0")
    B = Q.shape[0]
    i8 = mp.p.prec == I8
    oi = torch.full((B, stride), 7, dtype=torch.int32, device=dev)
    od = torch.zeros((B, stride), dtype=torch.float64 if i8 else torch.float32, device=dev)
    oc = torch.full((B,), 7, dtype=torch.int32, device=dev)
    mp.p.idx.search_batch_mixed_dev(torch.from_numpy(Q).to(dev), torch.from_numpy(ks.astype(np.int32)).to(dev), torch.from_numpy(efs.astype(np.int32)).to(dev),
                                    stride, ef_max, oi, od, oc,
                                    d_allow_lists=None if lists is None else torch.from_numpy(lists.view(np.int64)).to(dev),
                                    d_allow_of_query=None if of_q is None else torch.from_numpy(of_q).to(dev), dist64=i8, **flags)
    mp.p.idx.sync()
    return oi.cpu().numpy().view(np.uint32), od.cpu().numpy(), oc.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("name", ["f32_l2_640", "i8_cos_96"])
def test_mixed_dev_with_per_query_allow_lists(name):
    """kdb_search_batch_mixed_dev: every query its own key AND its own allow list (or none); per query the oracle's answer with both"""
    mp = _mp(name)
    p = mp.p
    B = 56
    L = _six_lists(p.n)
    qi, ks, efs = _batch(KEYS, B)
    rng = np.random.default_rng(9)
    of_q = rng.integers(-1, len(L), size=B).astype(np.int32)
    of_q[:7] = [-1, 0, 1, 2, 3, 4, 5]
    stride = int(ks.max())
    ids, dist, cnt = _dev_call(mp, p.Q[qi], ks, efs, stride, 1200, L, of_q, tie_flag=True, heap_order=True)
    assert not np.any(cnt >> 30)
    _check_padding(ids, dist, cnt, stride)
    for b in range(B):
        g = int(of_q[b])
        oi, od, _ = mp.oracle(int(qi[b]), int(ks[b]), int(efs[b]), None if g < 0 else L[g], g)
        c = int(cnt[b])
        where = (name, b, g, int(ks[b]), int(efs[b]))
        assert c == len(oi) and np.array_equal(ids[b, :c], oi), (where, ids[b, :c], oi)
        assert np.array_equal(p.scores(dist[b, :c]), od), where
    assert int(cnt[3 + 1]) == 0 and int(cnt[5 + 1]) == 0      # (the empty list, the list that names no vector)
    # G == 0: one optional list for the whole batch, as kdb_search_batch_dev has it
    import torch
    ids, dist, cnt = _dev_call(mp, p.Q[qi], ks, efs, stride, 1200, L[1:2].reshape(-1), None, tie_flag=True, heap_order=True)
    assert torch.cuda.is_available()
    for b in range(B):
        oi, od, _ = mp.oracle(int(qi[b]), int(ks[b]), int(efs[b]), L[1], 1)
        c = int(cnt[b])
        assert c == len(oi) and np.array_equal(ids[b, :c], oi) and np.array_equal(p.scores(dist[b, :c]), od), (name, b, "one shared list")


def test_mixed_bounds():
    """a query outside the launch's bounds -- k == 0, k > k_stride, effective ef above the capacity -- comes back from the _dev call as
    count 0 | KDB_MIXED_BAD_QUERY, never walked, and its neighbours in the batch are answered as ever; the host call, which can read
    the arrays, refuses the batch before anything is launched"""
    mp = _mp("f32_l2_640")
    p, hip = mp.p, mp.p.hip
    B, stride, ef_max = 16, 10, 64
    ks = np.array([10, 5, 0, 1, 11, 10, 10, 10, 0, 10, 3, 64, 10, 5, 10, 1], dtype=np.uint32)
    efs = np.array([16, 64, 16, 1, 16, 65, 0, 64, 0, 300, 7, 64, 16, 0, 1200, 0], dtype=np.uint32)
    bad = np.array([0, 0, 1, 0, 1, 1, 0, 0, 1, 1, 0, 1, 0, 0, 1, 0], dtype=bool)  # written down: k == 0 | k > 10 | max(ef, k) > 64
    qi = np.arange(B) % NQ
    ids, dist, cnt = _dev_call(mp, p.Q[qi], ks, efs, stride, ef_max, tie_flag=True, heap_order=True)
    shape = p.idx.launch_shape()[0]
    assert (shape["search"], shape["B"], shape["bs"]) == (1, B, 1), shape
    _check_padding(ids, dist, cnt, stride)
    for b in range(B):
        if bad[b]:
            assert int(cnt[b]) == hip.index.MIXED_BAD_QUERY, (b, hex(int(cnt[b])))
            continue
        oi, od, _ = mp.oracle(int(qi[b]), int(ks[b]), int(efs[b]))
        c = int(cnt[b])
        assert c == len(oi) and np.array_equal(ids[b, :c], oi) and np.array_equal(p.scores(dist[b, :c]), od), b
    # the host call: KDB_ERR_INVALID for k == 0 and for k > k_stride, nothing launched
    before = (p.idx.counters(), p.idx.launch_shape()[0])
    for sel in (slice(0, 3), slice(3, 5)):       # (..., k == 0) and (..., k == 11)
        with pytest.raises(hip.KdbError, match=r"status -1"):
            p.idx.search_batch_mixed(p.Q[qi][sel], ks[sel], efs[sel], k_stride=stride)
    assert (p.idx.counters(), p.idx.launch_shape()[0]) == before
    # ... and an effective ef above every other one is no error there: the host sizes the launch from the arrays
    ok = ~bad
    ok[[5, 9, 14]] = True
    ids, dist, cnt = p.idx.search_batch_mixed(p.Q[qi][ok], ks[ok], efs[ok], k_stride=stride, tie_flag=True, heap_order=True)
    assert p.idx.launch_shape()[0]["bs"] == 0 and not np.any(cnt >> 30)
    for j, b in enumerate(np.nonzero(ok)[0]):
        oi, od, _ = mp.oracle(int(qi[b]), int(ks[b]), int(efs[b]))
        c = int(cnt[j])
        assert c == len(oi) and np.array_equal(ids[j, :c], oi) and np.array_equal(p.scores(dist[j, :c]), od), b


def test_mixed_statistics_count_launches_with_distinct_keys():
    mp = _mp("f16_l2_96")
    p = mp.p
    s0 = p.idx.mixed_stats()
    p.idx.search_batch_mixed(p.Q[:4], [10, 10, 10, 10], [16, 16, 16, 16])          # one key: not a mixed launch
    assert p.idx.mixed_stats() == s0
    p.idx.search_batch_mixed(p.Q[:4], [10, 10, 10, 10], [10, 0, 5, 10])            # ... nor this one: max(ef, k) is 10 four times
    assert p.idx.mixed_stats() == s0
    p.idx.search_batch_mixed(p.Q[:4], [10, 10, 10, 10], [16, 0, 10, 5])            # 16, 10, 10, 10
    s1 = p.idx.mixed_stats()
    assert (s1[0], s1[1]) == (s0[0] + 1, s0[1] + 1) and s1[3] == 0
    p.idx.search_batch_mixed(p.Q[:4], [10, 5, 10, 10], [16, 16, 16, 16])
    s2 = p.idx.mixed_stats()
    assert (s2[0], s2[1]) == (s1[0] + 1, s1[1] + 1)


def test_mixed_on_an_empty_index_and_on_an_index_without_a_graph():
    """exactly as kdb_search_batch on the same handle: an empty index answers every query with count 0; rows without a graph are
    answered the way kdb_search_batch answers them on the same handle (no results, or KDB_ERR_STATE)"""
    import kektordb_amd as hip
    idx = hip.HipIndex(96, L2, F32, 16, 20, capacity=64)
    Q = np.random.default_rng(3).standard_normal((5, 96)).astype(np.float32)
    ks, efs = np.array([1, 10, 5, 10, 3], np.uint32), np.array([1, 0, 64, 300, 7], np.uint32)

    def outcome(call):
        try:
            ids, dist, cnt = call()
        except hip.KdbError as e:
            return str(e).split(":")[0]            # "... failed (status N)"
        assert not ids.any()
        return [int(c) for c in cnt]

    assert outcome(lambda: idx.search_batch_mixed(Q, ks, efs)) == [0] * 5 == outcome(lambda: idx.search_batch(Q, 10, 64))
    idx.upload_rows(np.random.default_rng(4).standard_normal((40, 96)).astype(np.float32), 1)
    idx.set_count(40)
    plain = outcome(lambda: idx.search_batch(Q, 10, 64))
    mixed = outcome(lambda: idx.search_batch_mixed(Q, ks, efs))
    assert mixed == plain or (isinstance(plain, str) and mixed == plain.replace("kdb_search_batch", "kdb_search_batch_mixed")), (plain, mixed)
    idx.Close()


CALLER_KEYS = [(10, 48), (5, 20), (20, 64), (10, 100), (3, 130)]


def test_concurrent_callers_with_different_keys_share_launches(oracle, hip, monkeypatch):
    """24 threads make one-query kdb_search_batch calls on ONE handle with keys drawn from five (k, ef) over three beam classes, every
    third call with the heap-order flag (the corpus has duplicate rows): every answer equals the same query's answer in a single
    homogeneous batch, some launches carried more than one key, and the calls shared launches.  The same traffic on a handle created
    under KDB_COMBINE_MIXED=0 gets equal answers from launches of one key each."""
    import threading
    from test_gpu_parity import build_pair
    n, dim = 6000, 96
    X = make_corpus_normal(n, dim)
    X[100:140] = X[99]
    Q = make_corpus_normal(192, dim, seed=502)
    Q[:8] = X[99] + 1e-3 * Q[:8]
    orc = graph = None
    for combine in ("1", "0"):
        monkeypatch.setenv("KDB_SLOTS", "2")
        monkeypatch.setenv("KDB_COMBINE_MIXED", combine)
        if orc is None:
            orc, idx = build_pair(oracle, hip, X, 1, efc=60)
            graph = orc.export_graph()
        else:
            idx = hip.HipIndex(dim, 1, 0, 16, 60, capacity=n + 8)
            idx.upload_rows(orc.rows()[1:], 1)
            idx.upload_graph_obj(graph)
        monkeypatch.delenv("KDB_SLOTS")
        monkeypatch.delenv("KDB_COMBINE_MIXED")
        want = {(key, h): idx.search_batch(Q, key[0], key[1], heap_order=h) for key in CALLER_KEYS for h in (False, True)}
        s0, m0 = idx.caller_stats(), idx.mixed_stats()
        errors = []

        def caller(t):
            try:
                rng = np.random.default_rng(1000 + t)
                for it in range(40):
                    b = (t * 40 + it) % Q.shape[0]
                    key = CALLER_KEYS[int(rng.integers(len(CALLER_KEYS)))]
                    h = it % 3 == 2
                    got = idx.search_batch(Q[b:b + 1], key[0], key[1], heap_order=h)
                    for a, r in zip(got, want[(key, h)]):
                        assert np.array_equal(a, r[b:b + 1]), (t, it, key, h, a, r[b:b + 1])
            except Exception as e:  # pragma: no cover - reported below
                errors.append(repr(e))

        ts = [threading.Thread(target=caller, args=(t,)) for t in range(24)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        assert not errors, (combine, errors[:3])
        s1, m1 = idx.caller_stats(), idx.mixed_stats()
        print(f"KDB_COMBINE_MIXED={combine}: launches {s1['launches'] - s0['launches']} for {s1['calls'] - s0['calls']} calls, largest {s1['largest']}, "
              f"mixed stats {[a - b for a, b in zip(m1, m0)]}")
        assert s1["slots"] == 2 and s1["calls"] - s0["calls"] == 24 * 40
        assert s1["launches"] - s0["launches"] < 24 * 40, "no call shared a launch"
        if combine == "1":
            assert m1[0] - m0[0] > 0 and m1[1] - m0[1] >= 2 * (m1[0] - m0[0]), (m0, m1)
        else:
            assert m1[0] == 0 and m1[1] == 0, m1
        idx.close()


def make_corpus_normal(n, dim, seed=501):
    from conftest import make_corpus
    return make_corpus(n, dim, "normal", seed=seed)
