"""BM25 text search and hybrid fusion on the device (text.hip) against a plain-Python restatement of DB.FindIDsByTextSearch
(pkg/core/core.go:2069-2190) and of the fusion in searchWithFusion (pkg/engine/ops.go:1072-1098, :1189-1207): dicts, Python floats,
math.log, the formulas in the reference's order.  Bars: bit for bit -- only correctly rounded double + * / occur."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NO = 0xFFFFFFFF


def bm25_ref(post, doc_len, total, avg, query, allowed=None):
    """every candidate of `query` (token ids) as (doc, score), by (score descending, id ascending); post: {token id: {doc: tf}}"""
    cand = {}
    for tok in query:
        for d, tf in post.get(tok, {}).items():
            cand.setdefault(d, {})[tok] = tf
    out = []
    for d, tfs in cand.items():
        if allowed is not None and not allowed(d):
            continue
        s = 0.0
        for tok in query:
            tf = tfs.get(tok, 0)
            if tok in post and tf and avg > 0:
                df = len(post[tok])
                idf = math.log(1 + (float(total) - float(df) + 0.5) / (float(df) + 0.5))
                s += idf * ((tf * 2.2) / (tf + 1.2 * (0.25 + 0.75 * (float(doc_len.get(d, 0)) / avg))))
        out.append((d, s))
    return sorted(out, key=lambda e: (-e[1], e[0]))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def snapshot_of(hip, post, doc_len, **kw):
    return hip.TextIndex({t: list(l.items()) for t, l in post.items()}, doc_len, **kw)


# ---- the text call ------------------------------------------------------------------------------------------------------------
N_IDS = 40000
TF = (1, 2, 7)


def text_corpus():
    rng = np.random.default_rng(7)
    lists = [range(1, 12301, 4),                      # 3075 documents over three full tiles, more than one 256-entry run per tile
             (4095, 4096, 4097, 8191, 8192),          # the tile seams
             range(30000, 30051),                     # far away: empty tiles in between
             (777,),                                  # a single document
             (N_IDS,),                                # the last id
             range(2, 9000, 7), range(5000, 5601)]
    lists += [sorted(rng.choice(np.arange(1, 20001), 200, replace=False).tolist()) for _ in range(5)]
    post = {t: {int(d): TF[int(d) % 3] for d in l} for t, l in enumerate(lists)}
    doc_len = {d: (d % 5) * 3 + 4 for l in post.values() for d in l}  # equal lengths and tfs: exact score ties
    return post, doc_len


QUERIES = [[0], [0, 5, 6], [5, 5, 1], [NO], [1, NO, 3], [], (list(range(12)) * 3)[:32], [2, 4], [1], [7, 8, 9, 10, 11]]
ALLOW = {"none": None, "third": lambda d: d % 3 == 0, "zero": lambda d: False}


@pytest.fixture(scope="module")
def text_index(hip):
    post, doc_len = text_corpus()
    idx = hip.HipIndex(4, hip.L2, hip.F32, capacity=N_IDS)
    idx.upload_rows(np.zeros((N_IDS, 4), dtype=np.float32), 1)
    idx.set_count(N_IDS)
    snap = snapshot_of(hip, post, doc_len, n_ids=N_IDS)
    idx.set_text(0, snap)
    ref = {name: [bm25_ref(post, doc_len, snap.total_docs, snap.avg_len, q, f) for q in QUERIES] for name, f in ALLOW.items()}
    yield idx, snap, post, doc_len, ref
    idx.close()


def allow_bitmap(f):
    if f is None:
        return None
    words = np.zeros((N_IDS >> 6) + 1, dtype=np.uint64)
    for d in range(1, N_IDS + 1):
        if f(d):
            words[d >> 6] |= np.uint64(1) << np.uint64(d & 63)
    return words


def check_text_answer(out, ref, k):
    ids, score, cnt, mx, nc = out
    for b, full in enumerate(ref):
        n = min(k, len(full))
        assert (int(cnt[b]), int(nc[b])) == (n, len(full)), b
        assert ids[b].tolist() == [d for d, _ in full[:n]] + [0] * (k - n), b
        assert bits(score[b]).tolist() == bits([s for _, s in full[:n]] + [0.0] * (k - n)).tolist(), b
        assert bits(mx[b]) == bits(full[0][1] if full else 0.0), b


@pytest.mark.parametrize("allow", sorted(ALLOW))
@pytest.mark.parametrize("k", [1, 10, 100, 1024])
def test_text_search(text_index, k, allow):
    idx, _, _, _, ref = text_index
    assert any(len(full) < 1024 for full in ref[allow]) and (allow != "none" or any(len(full) > 1024 for full in ref[allow]))
    check_text_answer(idx.text_search(0, QUERIES, k, allow_bitmap(ALLOW[allow])), ref[allow], k)


def test_text_search_dev(text_index, hip):
    import torch
    from kektordb_amd.index import pack_token_queries
    idx, _, _, _, ref = text_index
    k, B = 10, len(QUERIES)
    tok, nt = pack_token_queries(QUERIES)
    dev = lambda a: torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()
    ids, cnt, nc = (torch.zeros(s, dtype=torch.int32, device="cuda") for s in ((B, k), B, B))
    score, mx = (torch.zeros(s, dtype=torch.float64, device="cuda") for s in ((B, k), B))
    idx.text_search_dev(0, dev(tok), dev(nt), k, ids, score, cnt, mx, nc)
    idx.sync()
    check_text_answer((ids.cpu().numpy().view(np.uint32), score.cpu().numpy(), cnt.cpu().numpy(), mx.cpu().numpy(), nc.cpu().numpy()), ref["none"], k)


def test_zero_average_length_scores_zero_ordered_by_id(text_index, hip):
    idx, _, post, doc_len, _ = text_index
    idx.set_text(1, snapshot_of(hip, post, doc_len, n_ids=N_IDS, avg_len=0.0))
    ids, score, cnt, mx, nc = idx.text_search(1, [[0, 1]], 10)
    assert ids[0].tolist() == sorted(set(post[0]) | set(post[1]))[:10] and not bits(score).any() and bits(mx[0]) == 0
    assert (int(cnt[0]), int(nc[0])) == (10, len(set(post[0]) | set(post[1])))
    idx.drop_text(1)


def test_slots(text_index, hip):
    """what test_text_args.py cannot reach without an index: an id above the capacity, an empty slot, text_info after a refusal"""
    idx, snap, post, doc_len, _ = text_index
    before = idx.text_info(0)
    assert before[:2] == (len(post), sum(len(l) for l in post.values())) and idx.text_info(2) == (0, 0, 0)
    with pytest.raises(hip.KdbError, match="capacity"):
        idx.set_text(0, snapshot_of(hip, {0: {N_IDS + 1: 1}}, {N_IDS + 1: 3}))
    assert idx.text_info(0) == before
    with pytest.raises(hip.KdbError, match="no snapshot"):
        idx.text_search(2, [[0]], 5)
    with pytest.raises(hip.KdbError, match="no snapshot"):
        idx.hybrid_search(np.zeros((1, 4), dtype=np.float32), 5, 10, 2, [[0]])


# ---- the hybrid call ----------------------------------------------------------------------------------------------------------
HN, HDIM, HEF = 2000, 16, 64
H_TOKENS = [[0, 1], [2], [1, 2, 0], [], [NO], [0], [2, 2], [1, 0]]


@pytest.fixture(scope="module")
def hybrid_index(hip):
    rng = np.random.default_rng(11)
    X = rng.standard_normal((HN, HDIM)).astype(np.float32)
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    Q = (X[rng.choice(HN, len(H_TOKENS), replace=False)] + 0.05 * rng.standard_normal((len(H_TOKENS), HDIM))).astype(np.float32)
    post = {t: {int(d): TF[int(d) % 3] for d in rng.choice(np.arange(1, HN + 1), n, replace=False)} for t, n in enumerate((300, 150, 40))}
    doc_len = {d: 5 + (d * 7) % 23 for d in range(1, HN + 1)}
    idx = hip.HipIndex(HDIM, hip.COSINE, hip.F32, 16, 100, capacity=HN)
    idx.upload_rows(X, 1)
    idx.build(HN, batch=512, ef_construction=100, seed=3)
    snap = snapshot_of(hip, post, doc_len)
    idx.set_text(0, snap)
    full = [bm25_ref(post, doc_len, snap.total_docs, snap.avg_len, q) for q in H_TOKENS]
    yield idx, Q, full
    idx.close()


@pytest.mark.parametrize("k", [5, 50])
@pytest.mark.parametrize("alpha", [0.5, 0.3, 1.5])
def test_hybrid_search(hybrid_index, alpha, k):
    idx, Q, full = hybrid_index
    v_ids, v_dist, v_cnt = idx.search_batch(Q, k, HEF)  # the vector half: the library's own answers
    ids, score, cnt = idx.hybrid_search(Q, k, HEF, 0, H_TOKENS, alpha)
    a = alpha if 0 <= alpha <= 1 else 0.5
    below_cut = inside = outside = 0
    for b, toks in enumerate(H_TOKENS):
        vec = {int(v_ids[b, i]): 1.0 / (1.0 + (1.0 - float(v_dist[b, i]))) for i in range(int(v_cnt[b]))}
        if not toks:
            fused = dict(vec)
        else:
            mx = full[b][0][1] if full[b] else 0.0
            norm = {d: (s / mx if mx > 0 else s) for d, s in full[b]}
            assert len({(1 - a) * t for t in norm.values()}) == len(set(norm.values())), "two text scores collide after scaling: pick another seed"
            rank = {d: i for i, (d, _) in enumerate(full[b])}
            below_cut += sum(1 for d in vec if rank.get(d, -1) >= k)
            inside += sum(1 for d in vec if d in rank)
            outside += sum(1 for d in rank if d not in vec)
            fused = {d: a * v for d, v in vec.items()}
            for d, t in norm.items():
                fused[d] = fused.get(d, 0.0) + (1 - a) * t
        want = sorted(fused.items(), key=lambda e: (-e[1], e[0]))[:k]
        n = len(want)
        assert int(cnt[b]) == n, b
        assert ids[b].tolist() == [d for d, _ in want] + [0] * (k - n), b
        assert bits(score[b]).tolist() == bits([s for _, s in want] + [0.0] * (k - n)).tolist(), b
    assert below_cut and inside and outside, (below_cut, inside, outside)  # a condition on the inputs, like the one on collisions
