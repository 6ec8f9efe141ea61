"""The shard merge and the allow-list slice restated in plain numpy / Python -- the reference merge_topk_kernel (flat_scan.hip),
kdb_merge_topk / kdb_merge_topk_f64 (kdb_api_merge.hip) and slice_allow_kernel (cluster.hip) are pinned to.  Same role as filter_ref.py:
nothing of the library is used here.

The merge has no counterpart in the upstream project (it is single process); its definition is SURVEY section 8e: per query the
first `count` entries of every shard, ordered by (key, global id) with key = the raw value, or its negation where larger raw
values are nearer (dot products of the float32 cosine path), global id = id_base[g] + local id.
"""
import numpy as np

COUNT_TIED = 0x80000000   # bit 31 of a search's count (KDB_COUNT_TIED): carried, never part of the length
COUNT_MASK = 0x7fffffff


def merge_ref(negate, ids, dist, count, k, id_base=None):
    """ids / dist [G, B, k], count [G, B] (bit 31 may be set), id_base [G] or None.
    -> (ids [B, k] uint32, the ORIGINAL distances [B, k] in dist's dtype, count [B] uint32).  Behind the count: id 0, +Inf.  The
    merged count carries bit 31 iff any shard's count for that query did."""
    ids = np.asarray(ids, dtype=np.uint32)
    dist = np.asarray(dist)
    count = np.asarray(count, dtype=np.uint32)
    G, B = count.shape
    assert ids.shape == (G, B, k) and dist.shape == (G, B, k)
    base = np.zeros(G, dtype=np.uint64) if id_base is None else np.asarray(id_base, dtype=np.uint64)
    o_ids = np.zeros((B, k), dtype=np.uint32)
    o_dist = np.full((B, k), np.inf, dtype=dist.dtype)
    o_cnt = np.zeros(B, dtype=np.uint32)
    for q in range(B):
        gid, d = [], []
        tied = 0
        for g in range(G):
            c = int(count[g, q]) & COUNT_MASK
            assert c <= k
            tied |= int(count[g, q]) & COUNT_TIED
            gid.append(base[g] + ids[g, q, :c].astype(np.uint64))
            d.append(dist[g, q, :c])
        gid = np.concatenate(gid)
        d = np.concatenate(d)
        key = -d if negate else d               # in the input's dtype; -0.0 == 0.0, so those tie and the id decides
        order = np.lexsort((gid, key))[:k]      # primary key, then global id
        n = order.size
        o_ids[q, :n] = gid[order].astype(np.uint32)
        o_dist[q, :n] = d[order]
        o_cnt[q] = n | tied
    return o_ids, o_dist, o_cnt


def merge_lists(parts, id_base, k, dtype=np.float64):
    """merge_ref for ONE query whose shards answered with lists of their own lengths: parts = [(ids, dist), ...] (what the oracle's
    search / flat_scan return, an empty pair for a shard that contributes nothing).  -> (ids, dist) of the merged length."""
    G = len(parts)
    ids = np.zeros((G, 1, k), dtype=np.uint32)
    dist = np.full((G, 1, k), np.inf, dtype=dtype)
    cnt = np.zeros((G, 1), dtype=np.uint32)
    for g, (i, d) in enumerate(parts):
        n = len(i)
        assert n <= k
        ids[g, 0, :n] = i
        dist[g, 0, :n] = d
        cnt[g, 0] = n
    oi, od, oc = merge_ref(False, ids, dist, cnt, k, id_base)
    n = int(oc[0])
    return oi[0, :n], od[0, :n]


def slice_ref(allowed_global_ids, base, count):
    """The local allow list of the shard that owns global ids base + 1 .. base + count: uint64 words [(count >> 6) + 1], bit i of
    the list (word i >> 6, bit i & 63) set iff 1 <= i <= count and base + i is allowed.  Built id by id."""
    allowed = set(int(x) for x in allowed_global_ids)
    words = [0] * ((count >> 6) + 1)
    for i in range(1, count + 1):
        if base + i in allowed:
            words[i >> 6] |= 1 << (i & 63)
    return np.array(words, dtype=np.uint64)


def bitset_ids(words):
    """the ids a dense uint64 bitset names (bit 0 of word 0 = id 0), ascending"""
    out = []
    for w, v in enumerate(np.asarray(words, dtype=np.uint64).tolist()):
        while v:
            low = v & -v
            out.append(64 * w + low.bit_length() - 1)
            v ^= low
    return out
