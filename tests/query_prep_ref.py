"""numpy restatements of what searchInternal does to a query before it compares it with a row (hnsw_index.go:404-434), and the
query pools the query-preparation tests feed to both copies of that code on the device (no test in here).

  np_normalize      normalize() (:3034-3045): float32 sum of squares in index order (np.add.accumulate is a sequential sum), float64
                    sqrt, float32 reciprocal, float32 multiply; a sum that is not > 0 leaves the vector untouched
  np_f16_round_trip float16.Fromfloat32 and back: round to nearest even, 65520 and above to infinity
  np_quantize       Quantizer.Quantize (quantizer.go:150-176), from test_gpu_compress_edges (held against the oracle's there)
  np_prepared       the three in the reference's order for a (metric, precision)

numpy on the host keeps float32 denormals, as the reference's Go code does: a sum of squares of 1e-40 is > 0."""
import numpy as np

from test_gpu_compress_edges import QUANT_A, f16_pool, np_quantize  # noqa: F401 (the pools of the row-side tests, reused for queries)

L2, COSINE = 0, 1
F32, F16, I8 = 0, 1, 2


def np_normalize(q):
    q = np.asarray(q, dtype=np.float32)
    with np.errstate(all="ignore"):
        sq = q * q
        assert sq.dtype == np.float32
        nsq = np.add.accumulate(sq, dtype=np.float32)[-1]
        if not nsq > 0:
            return q.copy()
        inv = np.float32(1.0) / np.float32(np.sqrt(np.float64(nsq)))
        return q * inv


def np_f16_round_trip(q):
    with np.errstate(over="ignore"):
        return np.asarray(q, dtype=np.float32).astype(np.float16).astype(np.float32)


def np_prepared(q, metric, precision):
    """the float32 / float16 query a row is compared with, as float32 (int8: the normalised query, before Quantize)"""
    p = np_normalize(q) if metric == COSINE else np.asarray(q, dtype=np.float32).copy()
    return np_f16_round_trip(p) if precision == F16 else p


def same_bits(a, b):
    """float32 arrays equal bit for bit, except that the sign of a zero does not count (x * 1 + 0 * 0 turns -0.0 into +0.0)"""
    a = np.asarray(a, dtype=np.float32) + np.float32(0.0)
    b = np.asarray(b, dtype=np.float32) + np.float32(0.0)
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


def f32_query_pool(dim, seed=0):
    """name -> query: the values at which a normalisation goes wrong"""
    rng = np.random.default_rng(1000 * dim + seed)
    f = np.float32
    sign = rng.choice(np.array([-1.0, 1.0], f), dim)
    one_hot = np.zeros(dim, f)
    one_hot[dim // 2] = 3.5
    neg_zero = rng.standard_normal(dim).astype(f)
    neg_zero[::3] = -0.0
    pool = {
        "normal": rng.standard_normal(dim).astype(f),
        "zero": np.zeros(dim, f),
        "one_hot": one_hot,
        "denormal_sum": np.full(dim, 1e-20, f) * sign,                  # squares of 1e-40: the sum is a denormal > 0
        "underflow_sum": np.full(dim, 1e-23, f) * sign,                 # squares of 1e-46 are 0: the query stays un-normalised
        "overflow_sum_1e19": np.full(dim, 1e19, f) * sign,              # dim > 3: the sum is +Inf, the inverse 0, the query zeros
        "overflow_sum_2e19": np.full(dim, 2e19, f) * sign,              # ... at every dim
        "mixed_magnitudes": (10.0 ** rng.uniform(-18, 18, dim)).astype(f) * sign,
        "neg_zero": neg_zero,
    }
    with np.errstate(over="ignore", under="ignore"):
        nsq = {k: np.add.accumulate(v * v, dtype=f)[-1] for k, v in pool.items()}
    assert 0 < nsq["denormal_sum"] < f(1.17549435e-38) or dim > 117      # (118 squares of 1e-40 reach the smallest normal float)
    assert nsq["underflow_sum"] == 0 and np.isinf(nsq["overflow_sum_2e19"]) and (dim <= 3 or np.isinf(nsq["overflow_sum_1e19"]))
    assert not np_normalize(pool["overflow_sum_2e19"]).any() and np.array_equal(np_normalize(pool["underflow_sum"]), pool["underflow_sum"])
    assert np.signbit(np_normalize(neg_zero)[::3]).all()
    return pool


def f16_edge_values():
    """the float16 edge pool of the row-side tests that stays finite, plus the largest half, the largest float that still rounds to it
    and a value below half the smallest subnormal -- both signs"""
    more = np.array([65504, 65519.996, 1e-8], np.float32)
    c = np.concatenate([f16_pool(finite_small_only=True), more, -more])
    h = np_f16_round_trip(c)
    assert np.isfinite(h).all() and h[c == np.float32(65519.996)] == 65504 and h[c == np.float32(1e-8)] == 0
    return c


def i8_query_values():
    """float32 values whose quantisation with AbsMax QUANT_A reaches every int8 -127..127, lands on every k + 0.5 of both signs (and
    on its two float32 neighbours), clips at +-127, and lies beyond +-A up to x / A = inf"""
    A = QUANT_A
    j = np.arange(-127, 127)
    h = ((2 * j + 1) / 254.0 * float(A)).astype(np.float32)
    below_a = np.nextafter(A, np.float32(0))
    whole = (np.arange(-127, 128) / 127.0 * float(A)).astype(np.float32)
    vals = np.concatenate([h, np.nextafter(h, np.float32(np.inf)), np.nextafter(h, np.float32(-np.inf)), whole,
                           np.array([A, -A, below_a, -below_a, -0.0, 0.0, 1e-30, -1e-30, 1.17549435e-38, A / 2, -A / 254,
                                     1.5 * A, -2.0 * A, 3.0e30, -1.0e20, 3.0e38, -3.0e38], np.float32)])
    with np.errstate(over="ignore"):
        sc = (vals / A) * np.float32(127.0)
    inside = sc[np.abs(sc) < 127]
    ties = inside[np.abs(inside) * 2 % 2 == 1]                           # scaled values that are k + 0.5 exactly
    assert (ties > 0).sum() >= 20 and (ties < 0).sum() >= 20, "the pool must hold exact ties of both signs"
    assert set(np_quantize(vals, A).tolist()) == set(range(-127, 128))
    assert (np.abs(vals) > A).sum() >= 6 and np.isinf(sc).sum() == 2 and (np.abs(sc) == 127).any()
    return vals
