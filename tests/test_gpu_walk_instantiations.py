"""Walk parity, instantiation by instantiation: every (precision, metric, row width NCH, beam BS) cell of hnsw_search_kernel, in every
launch geometry launch_search_bs can pick for it, against the oracle's walk (ARITH_HIP_WAVE) bit for bit -- ids, distance bits,
n_dist, n_hops -- the way test_small_scan_chunk_instantiations walks through the exact scan's instantiations.

Each case reads back which kernel it ran (HipIndex.launch_shape, the kdb_probe_launch_shape test hook) and asserts that it is the
one the case was written for: a change of a register budget or an LDS footprint that moves a threshold between two geometries
fails here instead of silently taking a geometry out of the suite.

One oracle / HIP pair per (precision, metric, dim): the oracle builds the graph, both sides hold it.  2000 clustered rows, 30 of
them copies of one row (walks that meet equal distances: walked again in heap order), every 13th id soft-deleted (the pending list
is in play at every width).  12 queries -- six stored rows (the duplicated one among them), six fresh -- tiled up the ladder of
batch sizes; the first and the last 12 queries of every rung are compared, none left out: once under KDB_SEARCH_HEAP_ORDER (ids,
distance bits and counters of the oracle for every query, ties included) and once without it (the fast walk's own answer)."""
import functools

import numpy as np
import pytest

from conftest import make_corpus

pytestmark = pytest.mark.gpu

K = 10
N_DEFAULT = 2000      # rows per pair ...
# ... but for float16 x 1536 columns: the oracle's half -> float conversion makes that build the slowest by far (15 s at 2000 rows,
# efConstruction 20); 1400 rows take about 10 s and still leave more live nodes (1293) than the widest beam (ef 1200) holds
N_ROWS = {(1, 0, 1536): 1400}
EFC = 20      # (graph quality is not the matter here: a cheap build, the same graph on both sides)
NQ = 12
F32, F16, I8 = 0, 1, 2
L2, COS = 0, 1

# (precision, metric, dim) -> the NCH its walks must report.  Written down from search.hip / search_inst.hip, NOT computed from the
# code under test: 64 * NCH columns unrolled, 0 = the any-width loaders (640 columns: long rows on that path)
PAIRS = {
    (F32, L2, 256): 4, (F32, L2, 384): 6, (F32, L2, 512): 8, (F32, L2, 768): 12, (F32, L2, 1024): 16, (F32, L2, 1536): 24, (F32, L2, 640): 0,
    (F32, COS, 256): 4, (F32, COS, 384): 6, (F32, COS, 512): 8, (F32, COS, 768): 12, (F32, COS, 1024): 16, (F32, COS, 1536): 24, (F32, COS, 640): 0,
    (F16, L2, 96): 0, (F16, L2, 768): 12, (F16, L2, 1536): 24,
    (I8, COS, 96): 0, (I8, COS, 768): 12, (I8, COS, 1536): 24,
}
# the heap-order pass unrolls float32 rows of 768 / 1536 columns only (search_heap.hip heap_dispatch)
HEAP_NCH = {key: (nch if key[0] == F32 and nch in (12, 24) else 0) for key, nch in PAIRS.items()}

# ef -> (BS, words of the one-wave kernel's LDS hash (0: bitset), words of the latency modes' hash)
#   16 / 100 / 200: one, two, four register slots;  300 / 700: the LDS beam with the 8192- / 16384-word hash;  1200: the bitset only
BEAMS = {16: (1, 2048, 8192), 100: (2, 2048, 8192), 200: (4, 4096, 4096), 300: (0, 8192, 8192), 700: (0, 16384, 16384), 1200: (0, 0, 0)}
HASH, BITS = "hash", "bitset"
# the geometries (visited set, waves per query) a beam class must be seen in over its ladder
GEOMETRIES = {
    "reg": {(HASH, 4), (HASH, 2), (HASH, 1)},                       # register beams
    "lds": {(HASH, 4), (HASH, 2), (HASH, 1), (BITS, 1)},            # LDS beam, ef <= 1040: ... then the bitset for a batch too large for one round
    "bits": {(BITS, 4), (BITS, 2), (BITS, 1)},                      # ef 1200
}
LADDER = (12, 480, 2400, 8400)


def _class(ef):
    return "reg" if BEAMS[ef][0] else "lds" if BEAMS[ef][1] else "bits"


# What the hook reported on an MI355X (256 CUs; every threshold is 256 x resident workgroups of that kernel at that LDS size), batch
# sizes 256 .. 3072 in steps of 256, with these pairs' 153 soft-deleted nodes (156 entries of pending list in LDS):
#   * ef 16 / 100 (latency-mode hash 8192 words, 36 .. 42 KB of LDS per workgroup): four waves up to 1024 queries (768 at 640 and at
#     1536 columns of float32 / float16), one wave beyond;  two waves in (768, 1024] at 640 columns and at float16 x 1536 / ef 16 only
#   * ef 200 (hash 4096 words, 21 .. 27 KB): four waves up to 1024 (768 at 640 / 1536 columns, 1280 on int8 x 96 / 768), two waves up
#     to 1536 or 1792 (1024 at float16 x 1536), one wave beyond;  float32 x 768 / 1024: four waves up to 1024, then one
#   * ef 300 (large hash 8192 words, 38 .. 44 KB): four waves with the hash up to 1024 (768 at 640 / 1024 / 1536 columns), then the
#     bitset (four or two waves up to 1024 .. 2048, one wave beyond);  the hash with two waves in (768, 1024] at 640 columns only, with
#     one wave in (768, 1024] on int8 x 1536 only
#   * ef 700 (large hash 16384 words, 74 .. 80 KB): four waves with the hash up to 512, then the bitset (four waves up to 1024, two
#     up to 1536 .. 2048, one beyond)
#   * ef 1200 (bitset): four waves up to 1024 (768 at 640 / 1536 columns), two up to 1536 .. 2048 (1024 at float16 x 1536), one beyond;
#     float32 x 768 / 1024: four waves up to 1024, then one
# Extra rungs: where the ladder misses a geometry that a batch size does reach.  (cell, ef) -> batch sizes
EXTRA_RUNGS = {}
# Geometries no batch size reaches for a cell on this device, each with the line of launch_search_bs that excludes it.
UNREACHABLE = {}
_WHY_WIDE2 = ("`if (B <= wide2_max)` behind `if (B <= wide_max)`: the latency modes' footprint (over 32 KB with the 8192-word hash) lets "
              "LDS hold four workgroups per CU (three above 40 KB) whatever their wave count, and the four-wave kernel reaches that: wide2_max == wide_max")
_WHY_REGS2 = ("`if (B <= wide2_max)` (register beams) / `if (B <= ncu * occupancy_blocks(wk2, 128, wlds))` (bitset): the two-wave NCH 12 / 16 kernels' "
              "registers leave four workgroups per CU (kdb_search_minw: two waves per SIMD): the 1024 queries the four-wave kernel already takes")
_WHY_LDS_HASH = ("`if (B <= ncu * occupancy_blocks(wk2, 128, wlds))` and `if (B <= one_round)` behind the four-wave test of the LDS beam: with the "
                 "large hash a workgroup needs 38 .. 80 KB, LDS holds four (8192 words) or two (16384 words) per CU whatever their wave count, and "
                 "the four-wave kernel reaches that")
for _key in PAIRS:
    _prec, _metric, _dim = _key
    for _ef in (16, 100):
        if _dim == 640 or (_key == (F16, L2, 1536) and _ef == 16):
            EXTRA_RUNGS[_key + (_ef,)] = (1020,)
        else:
            UNREACHABLE[_key + (_ef,)] = ({(HASH, 2)}, _WHY_WIDE2)
    if _prec == F32 and _dim in (768, 1024):
        UNREACHABLE[_key + (200,)] = ({(HASH, 2)}, _WHY_REGS2)
        UNREACHABLE[_key + (1200,)] = ({(BITS, 2)}, _WHY_REGS2)
    else:
        EXTRA_RUNGS[_key + (200,)] = EXTRA_RUNGS[_key + (1200,)] = (1020,) if _key == (F16, L2, 1536) else (1536,)
    if _dim == 640:          # (the any-width four-wave kernel is compiled for three waves per SIMD: 768 queries, the two-wave one takes 1024)
        EXTRA_RUNGS[_key + (300,)] = (1020,)
        UNREACHABLE[_key + (300,)] = ({(HASH, 1)}, _WHY_LDS_HASH)
    elif _key == (I8, COS, 1536):   # (four and two waves: 768 queries; one wave per query fits four workgroups per CU)
        EXTRA_RUNGS[_key + (300,)] = (1020,)
        UNREACHABLE[_key + (300,)] = ({(HASH, 2)}, _WHY_LDS_HASH)
    else:
        UNREACHABLE[_key + (300,)] = ({(HASH, 2), (HASH, 1)}, _WHY_LDS_HASH)
    UNREACHABLE[_key + (700,)] = ({(HASH, 2), (HASH, 1)}, _WHY_LDS_HASH)


class Pair:
    def __init__(self, prec, metric, dim, walk_planes=True):
        import kektordb_amd as hip
        from oracle import oracle as O
        O.build()
        self.hip, self.O, self.prec, self.metric, self.dim = hip, O, prec, metric, dim
        N = self.n = N_ROWS.get((prec, metric, dim), N_DEFAULT)
        X = make_corpus(N, dim, "clustered", seed=700 + dim)
        dup = np.random.default_rng(1).choice(N, 30, replace=False)
        X[dup] = X[5]                                               # (the recipe of test_short_rows_of_the_published_shapes)
        self.deleted = list(range(13, N + 1, 13))
        orc = O.OracleIndex(dim, metric, prec, 16, EFC, seed=7)
        if prec == I8:
            orc.set_absmax(float(np.quantile(np.abs(X), 0.999)))    # (the quantiser of test_small_scan_chunk_instantiations)
        orc.add_many(X)
        for d in self.deleted:
            orc.mark_deleted(d)
        idx = hip.HipIndex(dim, metric, prec, 16, EFC, capacity=N + 8, walk_planes=walk_planes)
        idx.upload_rows(orc.rows()[1:], 1)
        if prec == I8:
            idx.upload_norms(orc.norms()[1:], 1)
            idx.set_quantizer(orc.absmax)
        idx.upload_graph_obj(orc.export_graph())
        orc.set_arith(O.ARITH_HIP_WAVE)
        self.orc, self.idx = orc, idx
        live = [i for i in range(N) if (i + 1) % 13 and i != 5 and i not in set(dup.tolist())]
        stored = [5] + live[100:1100:200]                           # six stored rows, the duplicated one first
        self.Q = np.concatenate([X[stored], make_corpus(NQ - 6, dim, "clustered", seed=701 + dim)]).astype(np.float32)
        assert self.Q.shape == (NQ, dim)
        rng = np.random.default_rng(dim)
        from kektordb_amd.index import dense_bitset
        allowed = np.nonzero(rng.random(N + 1) < 0.3)[0]
        self.allowed = set(int(a) for a in allowed if a >= 1)
        self.allow = dense_bitset(allowed[allowed >= 1], N)
        self._want = {}

    def want(self, ef, filtered):
        """the oracle's answers, computed once per (ef, filter) and left unchanged"""
        key = (ef, filtered)
        if key not in self._want:
            self._want[key] = [self.orc.search(self.Q[b], K, allow=self.allow if filtered else None, ef=ef, counters=True) for b in range(NQ)]
        return self._want[key]

    def scores(self, dist):
        if self.prec == F32:
            return np.array([self.idx.score(r) for r in dist], dtype=np.float64)
        return np.asarray(dist, dtype=np.float64)                   # float16: the float as it is; int8: the float64 the kernel wrote


@functools.lru_cache(maxsize=None)
def _pair(prec, metric, dim, walk_planes=True):
    return Pair(prec, metric, dim, walk_planes)


def _rungs(key, ef):
    return tuple(LADDER) + tuple(EXTRA_RUNGS.get(key + (ef,), ()))


def _walk_ladder(p, ef, nch, planes_ok, filtered=False):
    """every rung: the walk under test against the oracle on the first and the last 12 queries, and the kernel it reports"""
    hip, idx = p.hip, p.idx
    key = (p.prec, p.metric, p.dim)
    bs, hash1, hash_w = BEAMS[ef]
    want = p.want(ef, filtered)
    kw = {"dist64": True} if p.prec == I8 else {}
    seen = set()
    for B in _rungs(key, ef):
        Qb = np.tile(p.Q, (B // NQ, 1))
        ids, dist, cnt, (nd, nh) = idx.search_batch(Qb, K, ef, allow_bits=p.allow if filtered else None, trace=True, tie_flag=True, heap_order=True, **kw)
        s = idx.launch_shape()[0]
        print(f"shape prec={p.prec} metric={p.metric} dim={p.dim} ef={ef} filtered={int(filtered)} B={B}: {s}")
        assert (s["search"], s["B"]) == (1, B), s
        assert (s["prec"], s["metric"], s["nch"], s["bs"]) == (p.prec, p.metric, nch, bs), (key, ef, B, s)
        assert s["waves"] in (1, 2, 4) and s["vis_hash_words"] in ((0, hash1) if s["waves"] == 1 else (0, hash_w)), (key, ef, B, s)
        assert s["planes"] in ((0, 1) if planes_ok else (0,)) and (s["planes"] == 0 or (s["waves"] == 1 and bs != 0)), (key, ef, B, s)
        assert s["heap_pass"] == 1 and s["heap_nch"] == HEAP_NCH[key], (key, ef, B, s)
        assert (s["heap_hash_words"], s["heap_reg_results"]) == ({16: 2048, 100: 2048, 200: 4096}.get(ef, 0), int(ef == 16)), (key, ef, B, s)
        seen.add((HASH if s["vis_hash_words"] else BITS, s["waves"]))
        assert not np.any(cnt & hip.index.COUNT_TIED), (key, ef, B)             # heap order resolved every tie
        for b in list(range(NQ)) + list(range(B - NQ, B)):
            oi, od, (ond, onh) = want[b % NQ]
            c = int(cnt[b])
            assert c == len(oi) and np.array_equal(ids[b, :c], oi), (key, ef, B, b, ids[b, :c], oi)
            assert np.array_equal(p.scores(dist[b, :c]), od), (key, ef, B, b)
            assert (int(nd[b]), int(nh[b])) == (ond, onh), (key, ef, B, b, int(nd[b]), int(nh[b]), ond, onh)
            if filtered:
                assert set(ids[b, :c].tolist()) <= p.allowed
            assert not (set(ids[b, :c].tolist()) & set(p.deleted))
        # ... and the fast walk's OWN answer, no heap-order pass behind it.  (The copies of one row make every walk of a wide beam meet
        # equal distances -- all twelve queries from ef 700 on --, and the heap-order pass, which reads rows with the any-width loaders
        # outside float32 x 768 / 1536, then supplies the whole answer: a broken unrolled loader passed the comparison above at ef 700
        # and 1200.)  A query the walk does not flag is the oracle's walk as it stands; one it flags may order equal distances
        # otherwise -- the distance of every id it returns must still be the oracle's, bit for bit, and ascending
        ids, dist, cnt, (nd, nh) = idx.search_batch(Qb, K, ef, allow_bits=p.allow if filtered else None, trace=True, tie_flag=True, **kw)
        s1 = idx.launch_shape()[0]
        assert s1["heap_pass"] == 0 and all(s1[f] == s[f] for f in ("search", "prec", "metric", "nch", "bs", "vis_hash_words", "waves", "planes", "B")), (key, ef, B, s1, s)
        for b in list(range(NQ)) + list(range(B - NQ, B)):
            oi, od, (ond, onh) = want[b % NQ]
            c = int(cnt[b]) & int(hip.index.COUNT_MASK)
            got = p.scores(dist[b, :c])
            if int(cnt[b]) & int(hip.index.COUNT_TIED):
                assert c == len(oi) and np.all(ids[b, :c] >= 1), (key, ef, B, b)
                assert np.array_equal(got, p.orc.distances(p.Q[b % NQ], ids[b, :c])), (key, ef, B, b, "plain walk, tied")
                assert np.all(np.diff(got) >= 0), (key, ef, B, b)
            else:
                assert c == len(oi) and np.array_equal(ids[b, :c], oi), (key, ef, B, b, "plain walk")
                assert np.array_equal(got, od), (key, ef, B, b, "plain walk")
                assert (int(nd[b]), int(nh[b])) == (ond, onh), (key, ef, B, b, "plain walk")
    expected = GEOMETRIES[_class(ef)] - UNREACHABLE.get(key + (ef,), (set(), ""))[0]
    assert seen == expected, (key, ef, "geometries seen", sorted(seen), "expected", sorted(expected))
    return seen


CASES = [(prec, metric, dim, ef) for (prec, metric, dim) in PAIRS for ef in BEAMS]


@pytest.mark.parametrize("prec,metric,dim,ef", CASES)
def test_walk_instantiation(prec, metric, dim, ef):
    p = _pair(prec, metric, dim)
    nch = PAIRS[(prec, metric, dim)]
    planes_ok = (prec, metric, dim) == (F32, COS, 768)
    _walk_ladder(p, ef, nch, planes_ok)
    if ef == 100:
        # the heap pass had work: a plain call does flag at least one query
        kw = {"dist64": True} if prec == I8 else {}
        plain = p.idx.search_batch(p.Q, K, ef, tie_flag=True, **kw)
        assert np.any(plain[2] & p.hip.index.COUNT_TIED), (prec, metric, dim)
        assert p.idx.launch_shape()[0]["heap_pass"] == 0
        # the ladder again under a 30 % allow list, and once more behind finite garbage in every CU's LDS
        _walk_ladder(p, ef, nch, planes_ok, filtered=True)
        p.idx.poison_lds(0x5a5a5a5a)
        _walk_ladder(p, ef, nch, planes_ok)


@pytest.mark.parametrize("ef", list(BEAMS))
def test_walk_instantiation_768_cosine_without_planes(ef):
    """768-column cosine indexes walk their large batches on the planes kernel (its own module: test_gpu_walk_planes.py); a handle
    that opted out (KDB_INDEX_NO_WALK_PLANES) takes the plain NCH 12 kernel in every geometry"""
    p = _pair(F32, COS, 768, False)
    _walk_ladder(p, ef, 12, False)


def test_planes_kernel_is_what_large_768_cosine_batches_run():
    """(the other half of the pair of cases above: with planes allowed, the one-wave register-beam launches report the planes kernel)"""
    p = _pair(F32, COS, 768)
    for ef in (16, 100, 200):
        p.idx.search_batch(np.tile(p.Q, (LADDER[-1] // NQ, 1)), K, ef, trace=True)   # (traced: one launch, not staged chunks)
        s = p.idx.launch_shape()[0]
        assert (s["nch"], s["waves"], s["planes"], s["heap_pass"]) == (12, 1, 1, 0), (ef, s)
