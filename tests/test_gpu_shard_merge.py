"""The id-range shard at its headline shape -- eight shards behind one handle -- and at its edges, against tests/merge_ref.py.

A. the merge kernels alone (kdb_merge_topk_dev, kdb_merge_topk_packed_dev, kdb_merge_topk_packed_f64_dev) on the lists of
   test_merge_host.tie_heavy_lists: short lists, ties that only the global id decides, counts that carry KDB_COUNT_TIED, strides
   wider than the block, poison behind every count, outputs pre-filled with a sentinel;
B. eight shards of [64, 63, 1, 127, 192, 65, 700, 333] rows on one device through kdb_cluster_create: exact scan and walk against
   the merged oracle and against the shards' own answers;
C. the allow-list slice (slice_allow_kernel) at every word and shard border those sizes produce;
D. twelve consecutive calls that alternate the two lanes of a cluster, growing and shrinking, with and without a list;
E. KDB_SEARCH_TIE_FLAG through the cluster: a tied shard that answers with fewer than k entries.
Every comparison is exact: ids, distance bits, counts."""
import functools

import numpy as np
import pytest

from conftest import make_corpus
from merge_ref import COUNT_MASK, COUNT_TIED, merge_lists, merge_ref, slice_ref
from test_merge_host import MERGE_SHAPES, POISON32, SENT_CNT, SENT_ID, assert_merged, host_merge, tie_heavy_lists

pytestmark = pytest.mark.gpu

SIZES = (64, 63, 1, 127, 192, 65, 700, 333)
BASES = np.concatenate([[0], np.cumsum(SIZES)[:-1]]).astype(np.uint32)   # 0, 64, 127, 128, 255, 447, 512, 1212
N, DIM = int(sum(SIZES)), 32
SHARD_OF = np.repeat(np.arange(len(SIZES)), SIZES)                       # shard of row i (global id i + 1)
F64, TIE, HEAP = 8, 16, 32                                               # KDB_SEARCH_DIST_F64 / _TIE_FLAG / _HEAP_ORDER
CONFIGS = {"f32_l2": (0, 0), "f32_cosine": (1, 0), "i8_cosine": (1, 2), "f16_l2": (0, 1)}   # (metric, precision)


# ---------------------------------------------------------------------------------------------------------------------------
# A. the merge kernels alone
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def handles(hip):
    """what the merge entry points take their key direction (and stream) from: an L2 handle and a cosine / float32 one"""
    h = {False: hip.HipIndex(8, hip.L2, hip.F32, 16, 50, capacity=16), True: hip.HipIndex(8, hip.COSINE, hip.F32, 16, 50, capacity=16)}
    yield h
    for x in h.values():
        x.close()


def _cuda(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    elif a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(a).cuda()


def _outputs(B, k, dtype):
    """sentinels: a slot the kernel skips (a hole under a double write) keeps them"""
    return (_cuda(np.full((B, k), SENT_ID, dtype=np.uint32)), _cuda(np.full((B, k), -7.0, dtype=dtype)), _cuda(np.full(B, SENT_CNT, dtype=np.uint32)))


def _host(out):
    import torch
    torch.cuda.synchronize()
    oi, od, oc = out
    return oi.cpu().numpy().view(np.uint32), od.cpu().numpy(), oc.cpu().numpy().view(np.uint32)


def pack_blocks(ids, dist, count, extra):
    """the block one all-gather delivers, per shard: float32 ids | dist bits | count; float64 dist64 | ids | count | pad to an even
    length; then `extra` words.  Pad and extra words are POISON.  -> ([G, L] uint32, L)"""
    G, B, k = ids.shape
    bk = B * k
    if dist.dtype == np.float32:
        L = 2 * bk + B + extra
        blk = np.full((G, L), POISON32, dtype=np.uint32)
        blk[:, :bk] = ids.reshape(G, bk)
        blk[:, bk:2 * bk] = dist.reshape(G, bk).view(np.uint32)
        blk[:, 2 * bk:2 * bk + B] = count
    else:
        L = ((3 * bk + B + 1) & ~1) + extra
        blk = np.full((G, L), POISON32, dtype=np.uint32)
        blk[:, :2 * bk] = np.ascontiguousarray(dist.reshape(G, bk)).view(np.uint32)
        blk[:, 2 * bk:3 * bk] = ids.reshape(G, bk)
        blk[:, 3 * bk:3 * bk + B] = count
    return blk, L


def device_merges(idx, ids, dist, count, base, k):
    """every device route the lists can take -> {route: (ids, dist, count)}"""
    G, B = count.shape
    d_base = None if base is None else _cuda(base)
    got = {}
    if dist.dtype == np.float32:
        out = _outputs(B, k, np.float32)
        idx.merge_topk_dev(G, B, k, _cuda(ids), _cuda(dist), _cuda(count), d_base, *out)
        idx.sync()
        got["separate arrays"] = _host(out)
    for extra in (0, 6):
        blk, L = pack_blocks(ids, dist, count, extra)
        out = _outputs(B, k, dist.dtype)
        (idx.merge_topk_packed_dev if dist.dtype == np.float32 else idx.merge_topk_packed_f64_dev)(G, B, k, _cuda(blk), L, d_base, *out)
        idx.sync()
        got[f"packed, stride {L}"] = _host(out)
    return got


@pytest.mark.parametrize("G,k,B", MERGE_SHAPES)
def test_merge_kernels_against_the_reference(hip, handles, G, k, B):
    """G in {1, 2, 8} x k in {1, 10, 63, 64, 65, 100, 1024} (the e / k, e % k split over 64 lanes; odd B * k in the int8 block
    offsets), both key directions, id_base and NULL with disjoint ids, float32 and float64 lists"""
    for negate in (False, True):
        for disjoint in (False, True):
            ids, dist, count, base = tie_heavy_lists(G, B, k, negate, disjoint_ids=disjoint)
            want = merge_ref(negate, ids, dist, count, k, base)
            for route, got in device_merges(handles[negate], ids, dist, count, base, k).items():
                assert_merged(got, want, k, (route, "negate" if negate else "l2", "no id_base" if disjoint else "id_base"))
            assert_merged(host_merge(hip, negate, ids, dist, count, k, base), want, k, "host")
    for disjoint in (False, True):
        ids, dist, count, base = tie_heavy_lists(G, B, k, False, dtype=np.float64, disjoint_ids=disjoint)
        want = merge_ref(False, ids, dist, count, k, base)
        for route, got in device_merges(handles[False], ids, dist, count, base, k).items():
            assert_merged(got, want, k, (route, "f64", disjoint))
        assert_merged(host_merge(hip, False, ids, dist, count, k, base), want, k, "host f64")


# ---------------------------------------------------------------------------------------------------------------------------
# the eight shards
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def corpus(copies):
    """make_corpus(1545, 32, "normal"); with copies, 40 rows are overwritten with rows of OTHER shards: equal distances across
    shard borders.  -> (rows, the indices of the rows that were copied from)"""
    X = make_corpus(N, DIM, "normal", seed=191).copy()
    rng = np.random.default_rng(192)
    dst = rng.choice(N, 40, replace=False)
    src = []
    for d in dst:
        while True:
            s = int(rng.integers(0, N))
            if SHARD_OF[s] != SHARD_OF[d] and s not in dst:
                break
        src.append(s)
        if copies:
            X[d] = X[s]
    X.setflags(write=False)
    return X, np.array(src)


@functools.lru_cache(maxsize=None)
def queries(B):
    """the first third next to rows that have a copy in another shard, the rest anywhere"""
    X, src = corpus(True)
    Q = make_corpus(B, DIM, "normal", seed=193).copy()
    near = max(1, B // 3)
    Q[:near] = X[src[:near]] + np.float32(0.01) * make_corpus(near, DIM, "normal", seed=194)
    Q.setflags(write=False)
    return Q


def build_shards(hip, O, X, metric, prec, sizes=SIZES, efc=40):
    shards, orcs = [], []
    absmax = float(np.quantile(np.abs(X / np.linalg.norm(X, axis=1, keepdims=True)), 0.999)) if prec == O.I8 else None
    lo = 0
    for g, n in enumerate(sizes):
        orc = O.OracleIndex(DIM if X.shape[1] == DIM else X.shape[1], metric, prec, 16, efc, seed=3 + g)
        if prec == O.I8:
            orc.set_absmax(absmax)
        orc.add_many(X[lo:lo + n])
        idx = hip.HipIndex(X.shape[1], metric, prec, 16, efc, capacity=n + 8)
        idx.upload_rows(orc.rows()[1:], 1)
        if prec == O.I8:
            idx.upload_norms(orc.norms()[1:], 1)
            idx.set_quantizer(orc.absmax)
        idx.upload_graph_obj(orc.export_graph())
        orc.set_arith(O.ARITH_HIP_WAVE)
        shards.append(idx)
        orcs.append(orc)
        lo += n
    return shards, orcs


class World:
    """the clusters of this module, built once each: (configuration, with copies) -> (cluster, shards, oracles)"""

    def __init__(self, hip, O):
        self.hip, self.O, self.made = hip, O, {}

    def get(self, config, copies):
        if (config, copies) not in self.made:
            metric, prec = CONFIGS[config]
            shards, orcs = build_shards(self.hip, self.O, corpus(copies)[0], metric, prec)
            self.made[(config, copies)] = (self.hip.Cluster(shards, BASES), shards, orcs)
        return self.made[(config, copies)]

    def close(self):
        for cl, shards, _ in self.made.values():
            cl.close()
            for s in shards:
                s.close()


@pytest.fixture(scope="module")
def world(hip, oracle):
    w = World(hip, oracle)
    yield w
    w.close()


def scores(config, dist):
    """raw distances -> what the oracle reports (the reference's float64 epilogue)"""
    d = np.asarray(dist, dtype=np.float64)
    return 1.0 - d if config == "f32_cosine" else d


def expected(orcs, kind, Q, k, ef=0, allowed=None, bases=BASES):
    """per query the merged oracle answer: (ids, float64 scores).  allowed: None or the set of allowed GLOBAL ids; a shard whose
    slice (slice_ref) is empty contributes nothing"""
    slices = None if allowed is None else [slice_ref(allowed, int(b), o.count) for b, o in zip(bases, orcs)]
    none = (np.zeros(0, np.uint32), np.zeros(0))
    out = []
    for q in Q:
        parts = []
        for g, o in enumerate(orcs):
            a = None if slices is None else slices[g]
            if a is not None and not a.any():
                parts.append(none)
            else:
                parts.append(o.flat_scan(q, k, allow=a) if kind == "scan" else o.search(q, k, allow=a, ef=ef))
        out.append(merge_lists(parts, bases, k))
    return out


def assert_answers(config, got, want, what):
    ids, dist, cnt = got
    assert len(want) == ids.shape[0]
    for b, (wi, wd) in enumerate(want):
        c = int(cnt[b])
        assert c == len(wi), (what, b, c, len(wi))
        assert np.array_equal(ids[b, :c], wi), (what, b, ids[b, :c], wi)
        assert np.array_equal(scores(config, dist[b, :c]), wd), (what, b)
        assert np.all(ids[b, c:] == 0) and np.all(np.isposinf(dist[b, c:])), (what, b, "behind the count: id 0, +Inf")


def cross_shard_ties(ids, dist, cnt, bases=BASES):
    """neighbours of one distance that come from different shards"""
    n = 0
    for b in range(ids.shape[0]):
        c = int(cnt[b] & COUNT_MASK)
        if c < 2:
            continue
        shard = np.searchsorted(bases, ids[b, :c], side="left") - 1
        n += int(np.sum((dist[b, 1:c] == dist[b, :c - 1]) & (shard[1:] != shard[:-1])))
    return n


@pytest.mark.parametrize("config", list(CONFIGS))
def test_eight_shards_on_one_device(hip, world, config):
    """exact scan at k = 10 and k = 200 (more than five of the shards hold: short lists) on the corpus with copies, the walk at
    ef 80 on the corpus without; against the merged oracle, and the scan against merge_ref over the shards' own answers"""
    i8 = config == "i8_cosine"
    fl = F64 if i8 else 0
    cl, shards, orcs = world.get(config, True)
    assert cl.info() == {"shards": 8, "devices": 1, "shards_per_device": 8}
    Q = queries(12)
    for k in (10, 200):
        got = cl.flat_scan_batch(Q, k, flags=fl)
        assert_answers(config, got, expected(orcs, "scan", Q, k), (config, "scan", k))
        own = [s.flat_scan_batch(Q, k, dist64=i8) for s in shards]
        own_cnt = np.stack([o[2] for o in own])
        assert_merged(got, merge_ref(config == "f32_cosine", np.stack([o[0] for o in own]), np.stack([o[1] for o in own]), own_cnt, k, BASES),
                      k, (config, "scan of the shards themselves", k))
        assert int(np.sum(own_cnt[:, 0] < k)) == sum(n < k for n in SIZES)
        assert cross_shard_ties(*got) >= 3, "no equal distances across a shard border: the case does not test the order"
        if i8:   # without the flag: the float64 order, the doubles rounded on the way out
            i32, d32, c32 = cl.flat_scan_batch(Q, k)
            assert np.array_equal(i32, got[0]) and np.array_equal(d32, got[1].astype(np.float32)) and np.array_equal(c32, got[2])
    cl, shards, orcs = world.get(config, False)
    assert_answers(config, cl.search_batch(Q, 10, 80, flags=fl), expected(orcs, "walk", Q, 10, ef=80), (config, "walk"))


def test_eight_int8_shards_merge_doubles_that_share_a_float(hip, oracle, handles):
    """the rows of int8_collision_corpus in eight shards: distances that are distinct doubles and one float meet across shards.
    Cluster (float64 out and float32 out: one order), the packed float64 merge at both strides and the host merge, against
    merge_ref over the shards' own doubles and against the merged oracle"""
    from test_gpu_parity import INT8_CASE_ABSMAX, int8_collision_corpus
    O = oracle
    dim, k = 48, 100
    X, q = int8_collision_corpus(dim)
    per = -(-X.shape[0] // 8)
    sizes = [min(per, X.shape[0] - g * per) for g in range(8)]
    bases = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.uint32)
    shards, orcs = [], []
    for g, n in enumerate(sizes):
        orc = O.OracleIndex(dim, 1, O.I8, 16, 40, seed=7 + g)
        orc.set_absmax(INT8_CASE_ABSMAX)
        orc.add_batch(X[bases[g]:bases[g] + n])
        idx = hip.HipIndex(dim, 1, O.I8, 16, 40, capacity=n + 8)
        idx.upload_rows(orc.rows()[1:], 1)
        idx.upload_norms(orc.norms()[1:], 1)
        idx.set_quantizer(orc.absmax)
        idx.upload_graph_obj(orc.export_graph())
        shards.append(idx)
        orcs.append(orc)
    cl = hip.Cluster(shards, bases)
    Q = np.stack([q, q * np.float32(0.5), X[0], X[1]])
    got = cl.flat_scan_batch(Q, k, flags=F64)
    i32, d32, c32 = cl.flat_scan_batch(Q, k)
    assert got[1].dtype == np.float64 and d32.dtype == np.float32
    assert np.array_equal(i32, got[0]) and np.array_equal(d32, got[1].astype(np.float32)) and np.array_equal(c32, got[2])
    assert_answers("i8_cosine", got, expected(orcs, "scan", Q, k, bases=bases), "collision scan")
    own = [s.flat_scan_batch(Q, k, dist64=True) for s in shards]
    ids, dist, count = (np.stack([o[j] for o in own]) for j in range(3))
    want = merge_ref(False, ids, dist, count, k, bases)
    assert_merged(got, want, k, "cluster")
    for route, dev in device_merges(handles[False], ids, dist, count, bases, k).items():
        assert_merged(dev, want, k, route)
    assert_merged(host_merge(hip, False, ids, dist, count, k, bases), want, k, "host f64")
    turned = 0   # neighbours that are one float, distinct doubles, of different shards and in DESCENDING id order: a merge over floats swaps them
    for b in range(Q.shape[0]):
        wi, wd = want[0][b], want[1][b]
        f = wd.astype(np.float32)
        shard = np.searchsorted(bases, wi, side="left") - 1
        turned += int(np.sum((f[1:] == f[:-1]) & (wd[1:] != wd[:-1]) & (shard[1:] != shard[:-1]) & (wi[1:] < wi[:-1])))
    assert turned >= 1, "no float32 collision between distinct doubles of different shards: the case does not test the float64 merge"
    cl.close()
    for s in shards:
        s.close()


# ---------------------------------------------------------------------------------------------------------------------------
# C. allow-list slicing
# ---------------------------------------------------------------------------------------------------------------------------
WORDS = (N >> 6) + 1   # 25: exactly the corpus (bits 0 .. 1599)


def bitset(ids, words):
    """dense uint64 list of `words` words; ids at or above 64 * words do not fit and are left out"""
    w = [0] * words
    for i in ids:
        if i < 64 * words:
            w[i >> 6] |= 1 << (i & 63)
    return np.array(w, dtype=np.uint64)


def named(ids, words):
    """what a list of `words` words built from `ids` allows of the corpus"""
    return {int(i) for i in ids if 1 <= i <= N and i < 64 * words}


def edge_lists():
    """name -> set of global ids (ids outside [1, 1545] included: they must change nothing)"""
    first = {int(b) + 1 for b in BASES}
    last = {int(b) + n for b, n in zip(BASES, SIZES)}
    inner = {int(b) + j for b, n in zip(BASES, SIZES) for j in (63, 64, 65) if j <= n}
    outside = {0, N + 1, N + 5, 1599, 1600, 1700, 1855}      # bit 0; bits above 1545, within the corpus's last word and beyond it
    return {"edges": first | last | inner | outside, "first ids only": first | outside, "last ids only": last | {0}}


def test_allow_list_slices_at_word_and_shard_borders(hip, world):
    """bases with base & 63 in {0, 63, 60, ...}, counts with count & 63 in {0, 63, 1, 60, 13}, a shard of one row and one below 64;
    lists exactly as long as the corpus, 3 words short (the tail is denied) and 4 words long"""
    config = "f32_l2"
    cl, shards, orcs = world.get(config, True)
    clw, _, orcsw = world.get(config, False)
    Q = queries(6)
    k = 128
    for name, ids in edge_lists().items():
        for words in (WORDS, WORDS - 3, WORDS + 4):
            allowed = named(ids, words)
            assert 0 < len(allowed) < k
            got = cl.flat_scan_batch(Q, k, allow_bits=bitset(ids, words))
            for b in range(Q.shape[0]):
                assert set(got[0][b, :int(got[2][b])].tolist()) == allowed, (name, words, b)
                assert int(got[2][b]) == len(allowed)
            assert_answers(config, got, expected(orcs, "scan", Q, k, allowed=allowed), (name, words, "scan"))
            if name == "edges":
                gw = clw.search_batch(Q, 10, 80, allow_bits=bitset(ids, words))
                assert_answers(config, gw, expected(orcsw, "walk", Q, 10, ef=80, allowed=allowed), (name, words, "walk"))
    # a list that names ids, none of them in the corpus: nothing, from the scan as from the walk; a list that names NOTHING is no
    # filter for the exact scan (allowList.IsEmpty(), vector_index.go:130) and an answer without entries for the walk
    for got in (cl.flat_scan_batch(Q, 10, allow_bits=bitset({0, N + 1}, WORDS)), clw.search_batch(Q, 10, 80, allow_bits=bitset({0, N + 1}, WORDS)),
                clw.search_batch(Q, 10, 80, allow_bits=np.zeros(WORDS, np.uint64))):
        assert_answers(config, got, [(np.zeros(0, np.uint32), np.zeros(0))] * Q.shape[0], "nothing allowed")
    assert_answers(config, cl.flat_scan_batch(Q, 10, allow_bits=np.zeros(WORDS, np.uint64)), expected(orcs, "scan", Q, 10), "empty list, exact scan")
    rng = np.random.default_rng(195)
    Q = queries(12)
    for share in (0.1, 0.5):
        ids = np.nonzero(rng.random(64 * WORDS) < share)[0].tolist()
        allowed = named(ids, WORDS)
        ab = bitset(ids, WORDS)
        assert_answers(config, cl.flat_scan_batch(Q, 10, allow_bits=ab), expected(orcs, "scan", Q, 10, allowed=allowed), (share, "scan"))
        assert_answers(config, clw.search_batch(Q, 10, 80, allow_bits=ab), expected(orcsw, "walk", Q, 10, ef=80, allowed=allowed), (share, "walk"))


# ---------------------------------------------------------------------------------------------------------------------------
# D. lanes and growing buffers
# ---------------------------------------------------------------------------------------------------------------------------
def test_consecutive_calls_alternate_lanes_and_sizes(hip, world):
    """twelve calls on one cluster: even calls take lane 0, odd ones lane 1; every lane sees batches that grow and shrink, k from 1
    to 200, scans and walks, and a list after none and none after a list (a stale slice, a stale send slot or an answer offset
    of the previous plan would show)"""
    config = "f32_l2"
    cl, shards, orcs = world.get(config, False)
    rng = np.random.default_rng(196)
    lists = edge_lists()
    r10 = np.nonzero(rng.random(64 * WORDS) < 0.1)[0].tolist()
    r50 = np.nonzero(rng.random(64 * WORDS) < 0.5)[0].tolist()
    pool = queries(70)
    calls = [(3, 10, "scan", None, WORDS), (70, 200, "scan", lists["edges"], WORDS), (1, 1, "walk", None, WORDS),
             (40, 64, "scan", None, WORDS), (20, 10, "walk", r10, WORDS), (5, 10, "walk", r50, WORDS),
             (70, 200, "scan", None, WORDS), (2, 128, "scan", lists["edges"], WORDS - 3), (9, 10, "walk", lists["edges"], WORDS),
             (33, 65, "scan", r50, WORDS), (1, 1, "scan", lists["last ids only"], WORDS + 4), (12, 10, "walk", None, WORDS)]
    assert len(calls) == 12
    for n_call, (B, k, kind, ids, words) in enumerate(calls):
        Q = pool[(7 * n_call) % (70 - B + 1):][:B]
        ab = None if ids is None else bitset(ids, words)
        allowed = None if ids is None else named(ids, words)
        got = cl.flat_scan_batch(Q, k, allow_bits=ab) if kind == "scan" else cl.search_batch(Q, k, 80, allow_bits=ab)
        assert_answers(config, got, expected(orcs, kind, Q, k, ef=80, allowed=allowed), (n_call, B, k, kind))


# ---------------------------------------------------------------------------------------------------------------------------
# E. the tie flag through the cluster
# ---------------------------------------------------------------------------------------------------------------------------
def test_tie_flag_through_the_cluster(hip, oracle):
    """96 copies of one row dealt to the eight shards, queries next to it, and a list that leaves the small shards fewer than k
    answers: a shard then returns a SHORT list whose count carries KDB_COUNT_TIED.  The cluster's answer is merge_ref over the
    shards' own answers to the same flags, and its count carries bit 31 iff a shard's did"""
    O = oracle
    rng = np.random.default_rng(197)
    k, ef = 10, 80
    X = make_corpus(N, DIM, "normal", seed=198).copy()
    row = make_corpus(1, DIM, "normal", seed=199)[0]
    dup = np.concatenate([int(b) + rng.choice(n, min(n, 8), replace=False) for b, n in zip(BASES, SIZES)] + [rng.choice(N, 40, replace=False)])
    X[dup] = row[None, :]
    Q = (row[None, :] + np.float32(0.02) * make_corpus(8, DIM, "normal", seed=200)).astype(np.float32)
    allowed = set((np.nonzero(rng.random(N) < 0.5)[0] + 1).tolist())
    for g in (0, 1, 5):   # the shards of 64, 63 and 65 rows keep six ids, copies among them
        ids_g = set(range(int(BASES[g]) + 1, int(BASES[g]) + SIZES[g] + 1))
        copies_g = sorted(ids_g & set((dup + 1).tolist()))
        allowed = (allowed - ids_g) | set(copies_g[:4]) | set(sorted(ids_g - set(copies_g))[:2])
    shards, orcs = build_shards(hip, O, X, 0, O.F32)
    cl = hip.Cluster(shards, BASES)
    ab = bitset(allowed, WORDS)
    slices = [slice_ref(allowed, int(b), n) for b, n in zip(BASES, SIZES)]
    for heap in (False, True):
        got = cl.search_batch(Q, k, ef, allow_bits=ab, flags=TIE | (HEAP if heap else 0))
        own = [s.search_batch(Q, k, ef, allow_bits=sl, tie_flag=True, heap_order=heap) for s, sl in zip(shards, slices)]
        ids, dist, count = (np.stack([o[j] for o in own]) for j in range(3))
        assert_merged(got, merge_ref(False, ids, dist, count, k, BASES), k, ("tie flag", "heap order" if heap else "id order"))
        assert np.array_equal((got[2] & COUNT_TIED) != 0, ((count & COUNT_TIED) != 0).any(axis=0))
        if not heap:
            short_and_tied = ((count & COUNT_TIED) != 0) & ((count & COUNT_MASK) < k)
            assert short_and_tied.any(), "no shard answered with a short list that carries the tie bit: the case tests nothing"
            assert cross_shard_ties(*got) >= 1
    cl.close()
    for s in shards:
        s.close()
