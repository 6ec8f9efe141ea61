"""kdb_index_compress at its edges: deleted nodes, the sampled branches of Quantizer.Train, Quantize and float16 edge values.

THE CONTRACT under test (include/kektor_hip.h above kdb_index_compress): the reference collects the vectors with
IterateRaw (hnsw_index.go:2817-2838), which skips deleted nodes, so
  * Train (quantizer.go:49-135) sees the LIVE rows of 1..count in ascending id order: the 10 000 threshold, targetSize, step and
    the break count positions of that list; no live row -> KDB_ERR_STATE;
  * every row 1..count is still converted / quantised and keeps its id;
  * the deleted bits and their count reach the new index in both graph modes; after KDB_COMPRESS_REBUILD_GRAPH the deleted ids
    are in the graph as tombstones (inserted, then marked again) and no search or scan returns one.

TWO REFERENCES, neither shares code with the kernels:
  (a) the oracle's orc_quantizer_train / orc_quantize / orc_int8_norm, fed the dense array of live rows;
  (b) numpy, below: np_train (sort |v| of the sampled live rows, index int(float64(N) * 0.999), clamped), np_quantize
      ((x / a) * 127 in float32, clipped, rounded half away from zero in float64), np_norms (sqrt of the int64 sum of squares as
      float32), astype(np.float16).
test_references_agree (no GPU) holds (a) == (b) bit for bit on every Train and Quantize input of this file; the GPU tests compare
the device with both.  Everything is compared for equality: no tolerance is involved except assert_same_results_tol's for the
order of int8 scan results inside a run of equal distances (4- and 8-column int8 rows collide by the thousand)."""
import ctypes as C
import functools

import numpy as np
import pytest

from conftest import assert_same_results_tol, make_corpus

L2, COSINE = 0, 1
F32, F16, I8 = 0, 1, 2


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def bits32(x):
    return int(np.float32(x).view(np.uint32))


# ---- reference (b): numpy ----------------------------------------------------------------------------------------------------------
def np_sample(total):
    """positions of the training set within the list of `total` live vectors (quantizer.go:63-94) -> (positions, step)"""
    if total <= 10000:
        return np.arange(total), 1
    target = min(max(total // 10, 10000), 25000)
    step = max(total // target, 1)
    return np.arange(0, total, step)[:target], step


def np_train(live_rows):
    v = np.sort(np.abs(live_rows[np_sample(live_rows.shape[0])[0]]).ravel())
    return np.float32(v[min(int(float(v.size) * 0.999), v.size - 1)])


def np_quantize(X, a):
    a = np.float32(a)
    if a == 0:
        return np.zeros(X.shape, np.int8)
    with np.errstate(over="ignore"):
        sc = (X.astype(np.float32) / a) * np.float32(127.0)      # float32 throughout, as the reference
    assert sc.dtype == np.float32
    sc = np.clip(sc, np.float32(-127.0), np.float32(127.0)).astype(np.float64)
    return (np.sign(sc) * np.floor(np.abs(sc) + 0.5)).astype(np.int8)   # math.Round: half away from zero (exact in float64 here)


def np_norms(rows8):
    return np.sqrt((rows8.astype(np.int64) ** 2).sum(axis=1).astype(np.float64)).astype(np.float32)


# ---- reference (a): the oracle -----------------------------------------------------------------------------------------------------
def orc_train(O, live_rows):
    live_rows = np.ascontiguousarray(live_rows, dtype=np.float32)
    return np.float32(O.lib().orc_quantizer_train(_p(live_rows), live_rows.shape[0], live_rows.shape[1]))


def orc_quantize(O, X, a):
    X = np.ascontiguousarray(X, dtype=np.float32)
    out = np.zeros(X.shape, np.int8)
    O.lib().orc_quantize(_p(X), X.size, C.c_float(float(a)), _p(out))    # (element-wise: one call for the whole array)
    return out


def orc_norms(O, rows8):
    rows8 = np.ascontiguousarray(rows8)
    L = O.lib()
    return np.array([L.orc_int8_norm(_p(rows8[i]), rows8.shape[1]) for i in range(rows8.shape[0])], dtype=np.float32)


# ---- Train inputs ------------------------------------------------------------------------------------------------------------------
TRAIN_CASES = {  # name: (rows, dim, every k-th id is deleted (0: none), factor on the deleted rows, (live, step, sample size))
    "all_of_10000": (10000, 8, 0, 1.0, (10000, 1, 10000)),             # at the threshold: everything is used
    "first_10000_of_10001": (10001, 8, 0, 1.0, (10001, 1, 10000)),     # sampled with step 1, the break leaves the last row out
    "step_2": (20000, 8, 0, 1.0, (20000, 2, 10000)),
    "step_4": (44000, 8, 0, 1.0, (44000, 4, 10000)),
    "hardcap": (280000, 4, 13, 1.0, (258462, 10, 25000)),              # targetSize capped, the break fires
    "deletions_cross_the_threshold": (12000, 32, 5, 8.0, (9600, 1, 9600)),   # 12 000 rows are sampled, 9600 live ones are not
    "deletions_move_the_sample": (44000, 8, 22, 1.0, (42000, 4, 10000)),     # step 4 over the live LIST: other rows than ids 1, 5, ..
    "vacuumed": (3000, 32, 4, 8.0, (2250, 1, 2250)),                   # (the GPU test vacuums: the deleted rows become zero rows)
    "eight_magnitudes": (20000, 8, 0, 1.0, (20000, 2, 10000)),         # the order statistic lies inside a run of equal bit patterns
}
NEEDS_DIFFERENT_POPULATION = ("deletions_cross_the_threshold", "deletions_move_the_sample", "vacuumed")


@functools.lru_cache(maxsize=None)
def train_case(name):
    """-> (X float32 [n, dim]: the stored rows of ids 1..n, dead bool [n])"""
    n, dim, every, factor, _ = TRAIN_CASES[name]
    rng = np.random.default_rng(1000 + sorted(TRAIN_CASES).index(name))
    if name == "eight_magnitudes":   # four neighbouring floats and four others: the radix select's first three bytes decide little
        mags = (np.float32(0.3).view(np.uint32) + np.array([0, 1, 2, 3, 256, 65536, 1 << 20, 1 << 24], np.uint32)).view(np.float32)
        X = (rng.choice(mags, (n, dim)) * rng.choice(np.array([-1.0, 1.0], np.float32), (n, dim))).astype(np.float32)
    else:
        X = rng.standard_normal((n, dim), dtype=np.float32)
        X /= np.linalg.norm(X, axis=1, keepdims=True)
    dead = np.zeros(n, bool)
    if every:
        dead[every - 1::every] = True                                  # ids every, 2 * every, ...
        X[dead] *= np.float32(factor)
    X.setflags(write=False)
    dead.setflags(write=False)
    return X, dead


@functools.lru_cache(maxsize=None)
def train_expected(name):
    """both references on the case -> dict(a: AbsMax, a_all: the oracle's AbsMax over ALL rows, rows8, norms; stored: the rows the
    new index is made from -- for "vacuumed" the deleted rows are zero).  (a) == (b) is asserted by test_references_agree."""
    from oracle import oracle as O
    O.build()
    X, dead = train_case(name)
    stored = X
    if name == "vacuumed":
        stored = X.copy()
        stored[dead] = 0
    live = np.ascontiguousarray(stored[~dead])
    a_np, a_orc = np_train(live), orc_train(O, live)
    rows_np, rows_orc = np_quantize(stored, a_np), orc_quantize(O, stored, a_orc)
    return dict(a_np=a_np, a_orc=a_orc, a_all=orc_train(O, stored), a_all_before=orc_train(O, X), rows_np=rows_np, rows_orc=rows_orc,
                norms=np_norms(rows_np), stored=stored)


# ---- Quantize inputs ---------------------------------------------------------------------------------------------------------------
QUANT_ROWS = (1, 15, 16, 17, 63, 65)          # not multiples of the kernel's 16 rows per block / 4 rows per wave
QUANT_DIMS = (1, 3, 7, 17, 33, 100, 1000)     # row tails inside a 16-lane group, one column, more than one pass of the lanes
QUANT_A = np.float32(0.61803)                 # the AbsMax the rows are made for (no power of two: x / A rounds)


@functools.lru_cache(maxsize=None)
def quant_case(n, dim):
    """rows whose trained AbsMax is QUANT_A exactly: every |value| is <= A except the N - 1 - int(0.999 N) values that the quantile
    leaves above it (they clip), and A itself is present.  The pool: (2j + 1) / 254 * A for every j (the scaled value lands on or
    next to j + 0.5) and its two float32 neighbours, both signs; +-A and its neighbour below; -0.0, 0.0; +-1e-30; the smallest
    normal float."""
    A = QUANT_A
    N = n * dim
    qi = min(int(float(N) * 0.999), N - 1)
    nbig = N - 1 - qi
    j = np.arange(-127, 127)
    h = ((2 * j + 1) / 254.0 * float(A)).astype(np.float32)
    below_a = np.nextafter(A, np.float32(0))
    pool = np.concatenate([h, np.nextafter(h, np.float32(np.inf)), np.nextafter(h, np.float32(-np.inf)),
                           np.array([A, -A, below_a, -below_a, -0.0, 0.0, 1e-30, -1e-30, 1.17549435e-38, A / 2, -A / 254], np.float32)])
    assert np.abs(pool).max() == A
    rng = np.random.default_rng(n * 10007 + dim)
    vals = np.resize(rng.permutation(pool), N).astype(np.float32)
    pos = rng.permutation(N)
    vals[pos[0]] = A                                                # (N == 1: the only value)
    if N > 1:
        vals[pos[1]] = -A
    big = np.array([1.5 * A, -2.0 * A, 3.0e30, -1.0e20, 3.0e38, -3.0e38], np.float32)   # beyond +-A: clipped (x / A of the last two is inf)
    assert nbig + 2 <= N or nbig == 0
    vals[pos[2:2 + nbig]] = np.resize(big, nbig)
    X = vals.reshape(n, dim)
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def zero_quantizer_case():
    """65 x 100 with 5 non-zero values (fewer than 0.1 %): the 99.9th percentile is 0"""
    X = np.zeros((65, 100), np.float32)
    X[[0, 7, 16, 40, 64], [0, 99, 50, 3, 99]] = [0.5, -0.25, 1.0, -1.0, 1e-30]
    X[5, 5] = -0.0
    X.setflags(write=False)
    return X


# ---- float16 inputs ----------------------------------------------------------------------------------------------------------------
def f16_pool(finite_small_only=False):
    f = np.float32
    up = lambda x: np.nextafter(f(x), f(np.inf))
    dn = lambda x: np.nextafter(f(x), f(-np.inf))
    small = [f(6.1035e-5), f(2.0 ** -14), up(2.0 ** -14), dn(2.0 ** -14),          # the normal / subnormal border and its neighbours
             f(2.0 ** -14 - 2.0 ** -24), f(2.0 ** -14 - 2.0 ** -25), dn(2.0 ** -14 - 2.0 ** -25), up(2.0 ** -14 - 2.0 ** -25),
             f(2.0 ** -24), f(2.0 ** -25), up(2.0 ** -25), dn(2.0 ** -25), f(3 * 2.0 ** -25), up(3 * 2.0 ** -25), dn(3 * 2.0 ** -25),
             f(1e-30), f(1.17549435e-38), f(1e-40), f(0.0), f(-0.0),
             f(1 + 2.0 ** -11), up(1 + 2.0 ** -11), dn(1 + 2.0 ** -11), f(1 + 3 * 2.0 ** -11), f(0.1), f(1 / 3), f(2.5)]
    if finite_small_only:
        return np.array(small + [-x for x in small], np.float32)
    large = [f(65504), f(65519.99), f(65520), dn(65520), up(65504), f(1e6), f(3e38), f(np.inf)]
    return np.array(small + large + [-x for x in small + large] + [np.nan, np.float32(np.uint32(0x7f800001).view(np.float32)),
                                                                    np.uint32(0xffc12345).view(np.float32)], np.float32)


@functools.lru_cache(maxsize=None)
def f16_case(n, dim):
    pool = f16_pool()
    rng = np.random.default_rng(n * 131 + dim)
    X = np.resize(rng.permutation(pool), n * dim).astype(np.float32).reshape(n, dim)
    X.setflags(write=False)
    return X


# ---- CPU: the references against each other ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(TRAIN_CASES))
def test_references_agree_on_train_inputs(oracle, name):
    n, dim, every, factor, (want_live, want_step, want_nsel) = TRAIN_CASES[name]
    X, dead = train_case(name)
    e = train_expected(name)
    pos, step = np_sample(int((~dead).sum()))
    assert (int((~dead).sum()), step, pos.size) == (want_live, want_step, want_nsel)       # the branch the case is there for
    assert bits32(e["a_np"]) == bits32(e["a_orc"]) and e["a_np"] > 0
    assert np.array_equal(e["rows_np"], e["rows_orc"])
    assert np.abs(e["rows_np"]).max() == 127                                               # some values clip
    if name in NEEDS_DIFFERENT_POPULATION:                                                 # all rows train differently: the case can fail
        assert bits32(e["a_all"]) != bits32(e["a_np"]) and bits32(e["a_all_before"]) != bits32(e["a_np"])
        print(name, "AbsMax over the live rows", e["a_np"], "over all rows", e["a_all"], "over all rows before the vacuum", e["a_all_before"])
    if name == "eight_magnitudes":
        v = np.sort(np.abs(X[pos]).ravel())
        qi = int(float(v.size) * 0.999)
        assert v[qi] == v[qi - 1000] == v[-1] and np.unique(v).size == 8                   # inside a long run of equal values


@pytest.mark.parametrize("dim", QUANT_DIMS)
def test_references_agree_on_quantize_inputs(oracle, dim):
    O = oracle
    seen = set()
    for n in QUANT_ROWS:
        X = quant_case(n, dim)
        a_np, a_orc = np_train(X), orc_train(O, X)
        assert bits32(a_np) == bits32(a_orc) == bits32(QUANT_A)                            # the halves are halves of the TRAINED AbsMax
        r_np, r_orc = np_quantize(X, a_np), orc_quantize(O, X, a_orc)
        assert np.array_equal(r_np, r_orc)
        assert np.array_equal(np_norms(r_np).view(np.uint32), orc_norms(O, r_orc).view(np.uint32))
        seen |= set(np.unique(r_np).tolist())
        if n * dim > 1001:
            assert (np.abs(X) > QUANT_A).any()                                             # values beyond +-A that clip
    if dim >= 100:
        assert seen == set(range(-127, 128))
    Z = zero_quantizer_case()
    assert np_train(Z) == 0 and orc_train(O, Z) == 0 and (Z != 0).sum() < 0.001 * Z.size
    assert not np_quantize(Z, 0).any() and not orc_quantize(O, Z, 0.0).any()


def test_reference_rounding_and_float16_pool():
    """np_quantize itself, on values whose answer is known without it; the float16 pool holds what it is there for"""
    A = np.float32(1.0)
    x = np.array([0.5 / 127, -0.5 / 127, 1.5 / 127, 2.5 / 127, -2.5 / 127, 1.0, -1.0, 7.0, -7.0, -0.0, 1e-30], np.float64)
    x32 = x.astype(np.float32)
    sc = (x32 / A) * np.float32(127)
    want = [int(np.sign(s) * np.floor(abs(float(s)) + 0.5)) for s in np.clip(sc, -127, 127)]
    assert np_quantize(x32, A).tolist() == want and want[5:9] == [127, -127, 127, -127] and want[9:] == [0, 0]
    with np.errstate(over="ignore"):
        h = f16_pool().astype(np.float16)
    p = f16_pool()
    at = lambda v: h[np.nonzero(p.view(np.uint32) == np.float32(v).view(np.uint32))[0][0]]
    assert at(65504) == np.float16(65504) and np.isinf(at(65520)) and at(65519.99) == np.float16(65504) and np.isinf(at(1e6))
    assert at(2.0 ** -25) == 0 and at(np.nextafter(np.float32(2.0 ** -25), np.float32(1))).view(np.uint16) == 1
    assert at(2.0 ** -24).view(np.uint16) == 1 and at(-0.0).view(np.uint16) == 0x8000
    assert at(2.0 ** -14 - 2.0 ** -25).view(np.uint16) == 0x0400                           # a tie at the border: to even, the smallest normal
    assert np.isnan(h[np.isnan(p)]).all() and np.isnan(p).sum() == 3


# ---- GPU helpers -------------------------------------------------------------------------------------------------------------------
def bare_source(hip, X, metric, dead=None):
    """a float32 index without a graph: rows uploaded in stored form, count set, ids of `dead` (bool per row) marked deleted"""
    n, dim = X.shape
    src = hip.HipIndex(dim, metric, F32, 16, 60, capacity=n + 8)
    src.upload_rows(X, 1)
    src.set_count(n)
    if dead is not None and dead.any():
        src.Delete(np.nonzero(dead)[0] + 1)
    return src


def bare_graph(O, n, dead_ids):
    from kektordb_amd.index import dense_bitset
    return O.Graph(n, np.zeros(n + 1, np.uint8), 0, 1, [np.zeros(n + 2, np.uint64)], [np.zeros(0, np.uint32)], dense_bitset(dead_ids, n))


def check_int8_contents(O, dst, stored, a_refs, rows_refs):
    """AbsMax bits and every row against both references"""
    got_a = dst.quantizer_absmax()
    for a in a_refs:
        assert bits32(got_a) == bits32(a), (got_a, a)
    rows8 = dst.download_rows(1, stored.shape[0])
    for want in rows_refs:
        bad = np.nonzero((rows8 != want).any(axis=1))[0]
        assert bad.size == 0, (bad.size, "first differing row (id - 1)", int(bad[0]), rows8[bad[0]], want[bad[0]], stored[bad[0]])
    return rows8


def check_int8_norms_by_scan(O, dst, rows8, norms, a, dead, Q, k):
    """the stored norms through the exact scan's float64 distances (dot / (|q| * norm)): the oracle over the EXPECTED rows and
    norms answers the same, and no deleted id comes back"""
    n, dim = rows8.shape
    dead_ids = np.nonzero(dead)[0] + 1
    r1 = np.zeros((n + 1, dim), np.int8)
    r1[1:] = rows8
    nr = np.zeros(n + 1, np.float32)
    nr[1:] = norms
    orc = O.OracleIndex.from_graph(dim, O.COSINE, O.I8, 16, 60, r1, bare_graph(O, n, dead_ids), norms=nr, absmax=float(a))
    ids, dist, cnt = dst.flat_scan_batch(Q, k, dist64=True)
    for b in range(Q.shape[0]):
        oi, od = orc.flat_scan(Q[b], k)
        c = int(cnt[b])
        assert c == len(oi) == min(k, n - dead_ids.size)
        assert_same_results_tol(ids[b, :c], dist[b, :c], oi, od)
        assert not np.isin(ids[b, :c], dead_ids).any()


def queries_near(X, dead, nq, seed):
    rng = np.random.default_rng(seed)
    live = np.nonzero(~dead)[0]
    pick = rng.choice(live, nq, replace=False)
    return (X[pick] + 0.05 * rng.standard_normal((nq, X.shape[1]))).astype(np.float32)


# ---- GPU: Train --------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", [c for c in TRAIN_CASES if c != "vacuumed"])
def test_train_on_the_live_rows(oracle, hip, name):
    """cases 1-5 and the radix select inside a run of equal values: AbsMax, every row (deleted ones too, ids unchanged) and the
    norms, on an index without a graph"""
    X, dead = train_case(name)
    e = train_expected(name)
    src = bare_source(hip, X, COSINE, dead)
    dst = src.Compress(I8)
    rows8 = check_int8_contents(oracle, dst, X, (e["a_orc"], e["a_np"]), (e["rows_orc"], e["rows_np"]))
    check_int8_norms_by_scan(oracle, dst, rows8, e["norms"], e["a_np"], dead, queries_near(X, dead, 8, 5), 10)
    assert np.array_equal(src.download_rows(1, 16), X[:16])              # the source is left as it is


@pytest.mark.gpu
def test_train_after_a_vacuum_ignores_the_zeroed_rows(oracle, hip):
    """case 6: a quarter of 3000 x 32 deleted (rows scaled by 8), vacuumed -- the deleted rows are zero rows -- then compressed:
    AbsMax is the one of the live rows"""
    X, dead = train_case("vacuumed")
    e = train_expected("vacuumed")
    n, dim = X.shape
    src = hip.HipIndex(dim, COSINE, F32, 16, 60, capacity=n + 8)
    src.upload_rows(X, 1)
    src.build(n, batch=512, ef_construction=60, seed=3)
    src.Delete(np.nonzero(dead)[0] + 1)
    st = src.vacuum()
    assert st["dead_nodes"] == int(dead.sum()) == 750
    assert np.array_equal(src.download_rows(1, n), e["stored"])          # zero rows where the deleted ones were
    dst = src.Compress(I8)
    rows8 = check_int8_contents(oracle, dst, e["stored"], (e["a_orc"], e["a_np"]), (e["rows_orc"], e["rows_np"]))
    assert not rows8[dead].any()
    check_int8_norms_by_scan(oracle, dst, rows8, e["norms"], e["a_np"], dead, queries_near(X, dead, 8, 6), 10)
    ids, _, cnt = dst.search_batch(queries_near(X, dead, 8, 6), 10, 80)
    assert cnt.min() == 10 and not dead[ids.astype(np.int64) - 1].any()


@pytest.mark.gpu
@pytest.mark.parametrize("precision", [I8, F16])
def test_compress_with_every_node_deleted(hip, precision):
    """case 7: KDB_ERR_STATE (-5), as for an empty index (core.go:1168-1170)"""
    X = make_corpus(40, 8, "normal", seed=7)
    metric = COSINE if precision == I8 else L2
    src = bare_source(hip, X, metric, np.ones(40, bool))
    with pytest.raises(hip.KdbError) as err:
        src.Compress(precision)
    assert "status -5" in str(err.value), str(err.value)
    empty = hip.HipIndex(8, metric, F32, 16, 60, capacity=48)
    with pytest.raises(hip.KdbError) as err:
        empty.Compress(precision)
    assert "status -5" in str(err.value), str(err.value)


# ---- GPU: Quantize edge values -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dim", QUANT_DIMS)
def test_quantize_edge_values(oracle, hip, dim):
    """halves from both sides and with both signs, +-A, clipped values, -0.0, 1e-30, at row counts off the kernel's 16 rows per
    block and 4 rows per wave; the stored norms through one query per row (its own row answers at distance ~0)"""
    O = oracle
    for n in QUANT_ROWS:
        X = quant_case(n, dim)
        want_np, want_orc = np_quantize(X, QUANT_A), orc_quantize(O, X, QUANT_A)
        dst = bare_source(hip, X, COSINE).Compress(I8)
        rows8 = check_int8_contents(O, dst, X, (orc_train(O, X), np_train(X), QUANT_A), (want_orc, want_np))
        Q = rows8.astype(np.float32)
        Q[~Q.any(axis=1)] = 1.0                                           # (a zero row cannot be a query direction)
        check_int8_norms_by_scan(O, dst, rows8, orc_norms(O, want_orc), QUANT_A, np.zeros(n, bool), Q, min(n, 10))


@pytest.mark.gpu
def test_zero_quantizer(oracle, hip):
    """fewer than 0.1 % of the values are non-zero: AbsMax 0, every row zero (quantizer.go:155-157); the index is not searched"""
    Z = zero_quantizer_case()
    dst = bare_source(hip, Z, COSINE).Compress(I8)
    assert bits32(dst.quantizer_absmax()) == 0
    assert not dst.download_rows(1, Z.shape[0]).view(np.uint8).any()


# ---- GPU: float16 edge values ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dim", [1, 3, 33, 100])
def test_float16_edge_values(hip, dim):
    """65504, the RNE boundary to inf, 1e6, +-inf, -0.0, the normal / subnormal border, 2^-24, the tie 2^-25 -> 0, the float above
    it -> the smallest subnormal: bits equal astype(np.float16); a NaN stays a NaN"""
    for n in (1, 17):
        X = f16_case(n, dim)
        dst = bare_source(hip, X, L2).Compress(F16)
        got = dst.download_rows(1, n).view(np.uint16)
        with np.errstate(over="ignore"):
            want = X.astype(np.float16)
        nan = np.isnan(X)
        assert np.isnan(got.view(np.float16)[nan]).all()
        bad = np.nonzero((got != want.view(np.uint16)) & ~nan)
        assert bad[0].size == 0, (X[bad][:8], got[bad][:8], want.view(np.uint16)[bad][:8])


@pytest.mark.gpu
@pytest.mark.parametrize("B", [9, 70])
def test_float16_ranking_copy_on_edge_values(oracle, hip, B):
    """the same values (the finite ones that keep max ||x||^2 <= 1e4) through the half-precision RANKING copy of a float32 index:
    one exact scan, ranked on the copy, answers the oracle's exact scan bit for bit"""
    O = oracle
    n, dim, k = 600, 33, 10
    rng = np.random.default_rng(77)
    X = rng.standard_normal((n, dim), dtype=np.float32)
    pool = f16_pool(finite_small_only=True)
    mask = rng.random((n, dim)) < 0.4
    X[mask] = rng.choice(pool, int(mask.sum()))
    assert (X.astype(np.float64) ** 2).sum(axis=1).max() <= 1e4 and np.isfinite(X).all()
    src = bare_source(hip, X, L2)
    r1 = np.zeros((n + 1, dim), np.float32)
    r1[1:] = X
    orc = O.OracleIndex.from_graph(dim, O.L2, O.F32, 16, 60, r1, bare_graph(O, n, []))
    orc.set_arith(O.ARITH_HIP_WAVE)
    Q = (X[rng.choice(n, B, replace=False)] + 0.3 * rng.standard_normal((B, dim))).astype(np.float32)
    ids, dist, cnt = src.flat_scan_batch(Q, k)
    for b in range(B):
        oi, od = orc.flat_scan(Q[b], k)
        assert int(cnt[b]) == k == len(oi)
        assert np.array_equal(ids[b], oi), (b, ids[b], oi)
        assert np.array_equal(dist[b].astype(np.float64), od), b


# ---- GPU: deleted nodes through both graph modes -----------------------------------------------------------------------------------
GN, GDIM, GK = 4000, 64, 10


def graph_source(hip, precision):
    """a built float32 index of 4000 x 64 (int8: cosine, normalised rows; float16: L2) with 1000 ids deleted, the entry point
    among them -> (src, X, dead bool [n])"""
    X = make_corpus(GN, GDIM, "normal", seed=301 + precision)
    if precision == I8:
        X = (X / np.linalg.norm(X, axis=1, keepdims=True)).astype(np.float32)
    else:
        X = (X * 0.5).astype(np.float32)
    src = hip.HipIndex(GDIM, COSINE if precision == I8 else L2, F32, 16, 60, capacity=GN + 8)
    src.upload_rows(X, 1)
    src.build(GN, batch=512, ef_construction=60, seed=3)
    entry = src.graph_info()[1]
    rng = np.random.default_rng(5)
    others = rng.choice(np.setdiff1d(np.arange(1, GN + 1), [entry]), GN // 4 - 1, replace=False)
    dead = np.zeros(GN, bool)
    dead[others - 1] = True
    dead[entry - 1] = True
    src.Delete(np.nonzero(dead)[0] + 1)
    return src, X, dead


def expected_rows(O, precision, X, dead):
    """-> (rows [n + 1] in stored form for the oracle, norms or None, AbsMax or 0) by reference (a); (b) is asserted equal"""
    n, dim = X.shape
    if precision == F16:
        r1 = np.zeros((n + 1, dim), np.float16)
        r1[1:] = X.astype(np.float16)
        return r1.view(np.uint16), None, 0.0
    live = np.ascontiguousarray(X[~dead])
    a = orc_train(O, live)
    assert bits32(a) == bits32(np_train(live)) and bits32(a) != bits32(orc_train(O, X))   # (training on all rows would show)
    r1 = np.zeros((n + 1, dim), np.int8)
    r1[1:] = orc_quantize(O, X, a)
    assert np.array_equal(r1[1:], np_quantize(X, a))
    nr = np.zeros(n + 1, np.float32)
    nr[1:] = orc_norms(O, r1[1:])
    assert np.array_equal(nr[1:], np_norms(r1[1:]))
    return r1, nr, float(a)


def check_contents(precision, idx, r1, a):
    n = r1.shape[0] - 1
    got = idx.download_rows(1, n)
    assert np.array_equal(got.view(np.uint8), r1[1:].view(np.uint8))
    if precision == I8:
        assert bits32(idx.quantizer_absmax()) == bits32(a)


def check_deleted_bits(idx, dead, Q):
    """every id of D has its bit (a scan allowed to see nothing but D finds nothing), no other id has one (the census counts |D|)"""
    from kektordb_amd.index import dense_bitset
    D = np.nonzero(dead)[0] + 1
    only_d = idx.flat_scan_batch(Q, GK, allow_bits=dense_bitset(D, GN))
    assert not only_d[2].any()
    assert idx.dead_link_scan()[2] == D.size


def check_walks(O, precision, idx, r1, nr, a, dead, Q):
    """walks bit for bit (ids, distances, counters) against the oracle over (the index's downloaded graph, the deleted bits, the
    EXPECTED rows and norms); no deleted id in a walk or a scan"""
    from kektordb_amd.index import dense_bitset
    D = np.nonzero(dead)[0] + 1
    cnt, entry, ml, levels, offs, nbrs = idx.download_graph()
    g = O.Graph(cnt, levels, ml, entry, offs, nbrs, dense_bitset(D, cnt))
    if precision == I8:
        orc = O.OracleIndex.from_graph(GDIM, O.COSINE, O.I8, 16, 60, r1, g, norms=nr, absmax=a)
    else:
        orc = O.OracleIndex.from_graph(GDIM, O.L2, O.F16, 16, 60, r1, g)
        orc.set_arith(O.ARITH_HIP_WAVE)
    ids, dist, c, (nd, nh) = idx.search_batch(Q, GK, 80, trace=True, dist64=(precision == I8))
    fi, fd, fc = idx.flat_scan_batch(Q, GK)
    for b in range(Q.shape[0]):
        oi, od, (ond, onh) = orc.search(Q[b], GK, ef=80, counters=True)
        cb = int(c[b])
        assert cb == len(oi) == GK
        assert np.array_equal(ids[b, :cb], oi), (b, ids[b], oi)
        assert np.array_equal(dist[b, :cb].astype(np.float64), od), b
        assert (int(nd[b]), int(nh[b])) == (ond, onh), b
        assert int(fc[b]) == GK
    assert not dead[ids.astype(np.int64) - 1].any() and not dead[fi.astype(np.int64) - 1].any()


def graph_queries(precision, nq, seed):
    Q = make_corpus(nq, GDIM, "normal", seed=seed)
    return Q if precision == I8 else (Q * 0.5).astype(np.float32)


def recall_at_10(idx, Q):
    xi, _, _ = idx.flat_scan_batch(Q, GK)
    gi, _, _ = idx.search_batch(Q, GK, 80)
    return float(np.mean([len(set(gi[b].tolist()) & set(xi[b].tolist())) / GK for b in range(Q.shape[0])]))


@pytest.mark.gpu
@pytest.mark.parametrize("precision", [I8, F16])
def test_deleted_nodes_through_a_kept_graph(oracle, hip, precision):
    O = oracle
    src, X, dead = graph_source(hip, precision)
    r1, nr, a = expected_rows(O, precision, X, dead)
    dst = src.Compress(precision)
    check_contents(precision, dst, r1, a)
    gs, gd = src.download_graph(), dst.download_graph()
    assert gs[:3] == gd[:3] and np.array_equal(gs[3], gd[3])
    assert all(np.array_equal(x, y) for x, y in zip(gs[4], gd[4])) and all(np.array_equal(x, y) for x, y in zip(gs[5], gd[5]))
    Q = graph_queries(precision, 24, 302)
    check_deleted_bits(dst, dead, Q)
    s_ids, s_links, s_dead = src.dead_link_scan()
    d_ids, d_links, d_dead = dst.dead_link_scan()
    assert np.array_equal(s_ids, d_ids) and (s_links, s_dead) == (d_links, d_dead) and d_dead == GN // 4 and d_links > 0
    check_walks(O, precision, dst, r1, nr, a, dead, Q)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", [I8, F16])
def test_deleted_nodes_through_a_rebuilt_graph(oracle, hip, precision):
    O = oracle
    src, X, dead = graph_source(hip, precision)
    r1, nr, a = expected_rows(O, precision, X, dead)
    kept = src.Compress(precision)
    reb = src.Compress(precision, rebuild_graph=True)
    check_contents(precision, reb, r1, a)
    gk, gr = kept.download_graph(), reb.download_graph()
    assert gr[0] == GN and gr[2] >= 1
    assert not all(np.array_equal(x, y) for x, y in zip(gk[5], gr[5])), "the graph was not rebuilt"
    Q = graph_queries(precision, 24, 302)
    check_deleted_bits(reb, dead, Q)
    assert reb.dead_link_scan()[2] == 1000
    check_walks(O, precision, reb, r1, nr, a, dead, Q)
    Q2 = graph_queries(precision, 200, 303)
    for ix in (kept, reb):
        gi, _, gc = ix.search_batch(Q2, GK, 80)
        xi, _, xc = ix.flat_scan_batch(Q2, GK)
        assert gc.min() == GK == xc.min() and not dead[gi.astype(np.int64) - 1].any() and not dead[xi.astype(np.int64) - 1].any()
    rec = [recall_at_10(kept, Q2), recall_at_10(reb, Q2)]
    print("recall@10 at ef=80 with a quarter deleted (kept float32 graph, rebuilt graph):", rec)
    assert rec[1] >= rec[0] - 0.03, rec


@pytest.mark.gpu
@pytest.mark.parametrize("precision", [I8, F16])
def test_vacuum_after_a_rebuild(hip, precision):
    src, X, dead = graph_source(hip, precision)
    reb = src.Compress(precision, rebuild_graph=True)
    st = reb.vacuum()
    assert st["dead_nodes"] == 1000 and st["dead_links_found"] == st["dead_links_dropped"]
    assert st["nodes_repaired"] > 0 and not dead[st["entry"] - 1]
    again = reb.vacuum()
    assert (again["dead_nodes"], again["nodes_repaired"], again["lists_written"], again["dead_links_found"]) == (1000, 0, 0, 0)
    Q = graph_queries(precision, 24, 302)
    ids, _, cnt = reb.search_batch(Q, GK, 80)
    assert cnt.min() == GK and not dead[ids.astype(np.int64) - 1].any()
