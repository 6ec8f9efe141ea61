"""kdb_merge_topk / kdb_merge_topk_f64 (the host merge of the id-range shard, kdb_api_merge.hip) against merge_ref on lists made to
collide: few distinct distances, short lists, counts that carry KDB_COUNT_TIED, id bases that turn the local id order round.
No GPU: the two entry points are host code.  tie_heavy_lists is also what tests/test_gpu_shard_merge.py feeds the device merges."""
import numpy as np
import pytest

from merge_ref import COUNT_MASK, COUNT_TIED, merge_ref

POISON32 = 0xdeadbeef            # behind a shard's count: as a float -6.26e18 (first on the L2 path if it is ever read), as an id 3.7e9
POISON64 = 0xdeadbeefdeadbeef    # as a double -1.2e148
SENT_ID, SENT_CNT = 0xabababab, 0x55555555
VALUES = np.array([-1.5, -0.25, 0.0, 0.125, 0.5, 0.75, 2.0, 3.5])   # exact in float32


@pytest.fixture(scope="module")
def K():
    import kektordb_amd
    kektordb_amd.build_library()
    return kektordb_amd


def tie_heavy_lists(G, B, k, negate, dtype=np.float32, seed=0, disjoint_ids=False, tied_counts=True):
    """-> ids [G, B, k] uint32 (local, 1-based), dist [G, B, k], count [G, B] uint32, id_base [G] uint32 (None with disjoint_ids).
    Distances: eight values, sorted per list in key order, so most keys collide within and across shards; list 0 is all equal,
    list 1 ends in +Inf entries, list 2 mixes 0.0 and -0.0 (lists numbered g * B + q).  Counts from {0, 1, k - 1, k}; query 3 has
    every shard at 0 and query 4 a total below k (where B allows); with tied_counts a third of them carry bit 31.  Ids: unique
    within a list, from overlapping local ranges of which shard 0's is the HIGHEST, while id_base ascends -- the global order is
    the local one turned round.  Everything behind a count is POISON."""
    rng = np.random.default_rng(seed + 1000 * G + 7 * k + B + (500 if negate else 0))
    span = k + 6
    dist = rng.choice(VALUES, size=(G, B, k)).astype(dtype)
    for n_list in range(min(3, G * B)):
        g, q = divmod(n_list, B)
        if n_list == 0:
            dist[g, q, :] = dtype(0.5)
        elif n_list == 1:
            dist[g, q, k // 2:] = np.inf
        else:
            dist[g, q, :] = np.where(rng.random(k) < 0.5, dtype(0.0), dtype(-0.0))
    if B > 2:   # ... and so does every other shard's list of that query: whatever the key direction, the zeros ARE its answer
        dist[:, 2, :] = np.where(rng.random((G, k)) < 0.5, dtype(0.0), dtype(-0.0))
    dist = np.sort(dist, axis=2)
    if negate:
        dist = dist[:, :, ::-1].copy()
    ids = np.zeros((G, B, k), dtype=np.uint32)
    for g in range(G):
        for q in range(B):
            ids[g, q] = 1 + 3 * (G - 1 - g) + rng.permutation(span)[:k]
    base = (np.arange(G, dtype=np.uint32) * np.uint32(span + 3 * G + 11)).astype(np.uint32)
    count = rng.choice(np.array(sorted({0, 1, k - 1, k}), dtype=np.uint32), size=(G, B)).astype(np.uint32)
    for n_list in range(min(3, G * B)):       # the three special lists are full ones
        count[n_list // B, n_list % B] = k
    if B > 3:
        count[:, 3] = 0
    if B > 4:
        count[:, 4] = 0
        count[G - 1, 4] = min(1, k - 1)
    if tied_counts:
        count = np.where(rng.random((G, B)) < 0.34, count | np.uint32(COUNT_TIED), count).astype(np.uint32)
        if G * B > 1:
            g, q = divmod(G * B - 1, B)
            count[g, q] = np.uint32(k - 1) | np.uint32(COUNT_TIED)   # a short list that carries the bit, whatever the draw
    behind = np.arange(k)[None, None, :] >= (count & np.uint32(COUNT_MASK))[:, :, None]
    ids[behind] = POISON32
    if dtype == np.float32:
        dist.view(np.uint32)[behind] = POISON32
    else:
        dist.view(np.uint64)[behind] = POISON64
    if disjoint_ids:
        live = ~behind
        ids[live] = (ids + base[:, None, None])[live]
        return ids, dist, count, None
    return ids, dist, count, base


def assert_merged(got, want, k, what):
    """ids and distance BITS below the count, (0, +Inf) behind it, counts equal (bit 31 included)"""
    gi, gd, gc = got
    wi, wd, wc = want
    assert np.array_equal(gc, wc), (what, [hex(int(x)) for x in gc], [hex(int(x)) for x in wc])
    bits = np.uint32 if wd.dtype == np.float32 else np.uint64
    assert gd.dtype == wd.dtype
    assert np.array_equal(gi, wi), (what, np.nonzero(gi != wi))
    assert np.array_equal(gd.view(bits), wd.view(bits)), (what, np.nonzero(gd.view(bits) != wd.view(bits)))
    behind = np.arange(k)[None, :] >= (wc & np.uint32(COUNT_MASK))[:, None]
    assert np.all(gi[behind] == 0) and np.all(np.isposinf(gd[behind])), what


def host_merge(K, negate, ids, dist, count, k, base):
    """kektordb_amd.index.merge_topk into outputs that were pre-filled with a sentinel"""
    from kektordb_amd.index import merge_topk
    G, B = count.shape
    out = (np.full((B, k), SENT_ID, dtype=np.uint32), np.full((B, k), -7.0, dtype=dist.dtype), np.full(B, SENT_CNT, dtype=np.uint32))
    if dist.dtype == np.float64:
        return merge_topk(K.COSINE, ids, dist, count, k, id_base=base, precision=K.I8, out=out)
    return merge_topk(K.COSINE if negate else K.L2, ids, dist, count, k, id_base=base, precision=K.F32, out=out)


MERGE_SHAPES = [(G, k, 1 if k == 1024 else 5) for G in (1, 2, 8) for k in (1, 10, 63, 64, 65, 100, 1024)]


@pytest.mark.parametrize("G,k,B", MERGE_SHAPES)
def test_host_merge_against_the_reference(K, G, k, B):
    for negate in (False, True):
        for disjoint in (False, True):
            ids, dist, count, base = tie_heavy_lists(G, B, k, negate, disjoint_ids=disjoint)
            want = merge_ref(negate, ids, dist, count, k, base)
            assert_merged(host_merge(K, negate, ids, dist, count, k, base), want, k, ("f32", negate, disjoint))
    ids, dist, count, base = tie_heavy_lists(G, B, k, False, dtype=np.float64)
    assert_merged(host_merge(K, False, ids, dist, count, k, base), merge_ref(False, ids, dist, count, k, base), k, "f64")


def test_the_inputs_can_fail():
    """what the cases above claim to contain: ties across shards that only the GLOBAL id decides, against the local order; short
    lists, a query without answers and one with fewer than k; a short list whose count carries bit 31; merged counts with and
    without the bit; +Inf, 0.0 and -0.0 among the answers"""
    B, k = 5, 10
    TIED, MASK = np.uint32(COUNT_TIED), np.uint32(COUNT_MASK)
    merged_bits = set()
    for G in (2, 8):
        for negate in (False, True):
            ids, dist, count, base = tie_heavy_lists(G, B, k, negate)
            oi, od, oc = merge_ref(negate, ids, dist, count, k, base)
            c = count & MASK
            assert np.any(((count & TIED) != 0) & (c < k)) and np.any(((count & TIED) == 0) & (c < k)) and np.any(c == k)
            assert np.all(c[:, 3] == 0) and oc[3] & MASK == 0
            assert 0 < int(c[:, 4].sum()) < k and int(oc[4] & MASK) == int(c[:, 4].sum())
            merged_bits |= set(((oc & TIED) != 0).tolist())
            n_cross = n_turned = 0
            answers = []
            for q in range(B):
                n = int(oc[q] & MASK)
                answers.append(od[q, :n])
                if n < 2:
                    continue
                shard = np.searchsorted(base, oi[q, :n], side="left") - 1
                local = oi[q, :n] - base[shard]
                cross = (od[q, 1:n] == od[q, :n - 1]) & (shard[1:] != shard[:-1])
                n_cross += int(np.sum(cross))
                n_turned += int(np.sum(cross & (local[1:] < local[:-1])))   # a merge that ignored id_base would swap these
            assert G == 2 or (n_cross >= 5 and n_turned >= 2), (G, negate, n_cross, n_turned)
            a = np.concatenate(answers)
            assert np.any((a == 0.0) & ~np.signbit(a)) and np.any((a == 0.0) & np.signbit(a)), (G, negate)
            assert np.isposinf(a).any() or not negate, (G, negate)   # (+Inf is the nearest key only where keys are negated)
    assert merged_bits == {True, False}
