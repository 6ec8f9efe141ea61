"""BM25 with a query's id space split across workgroups (bm25_topk_kernel<true> + bm25_merge_kernel, kdb_text_split_plan) against the
plain-Python restatement of tests/test_gpu_text.py on that module's corpus (ten tiles, lists across the tile seams, empty tiles, a
list on the last id, exact score ties).  Bars: bit for bit, as there.  KDB_TEXT_SPLIT forces the split at these small shapes;
HipIndex.text_plan says, before every comparison, that the case really ran split."""
import numpy as np
import pytest

from kektordb_amd.index import pack_token_queries
from test_gpu_text import ALLOW, HDIM, N_IDS, QUERIES, TF, allow_bitmap, bm25_ref, check_text_answer, snapshot_of, text_corpus

pytestmark = pytest.mark.gpu

# [6, 3]: the longest list lies inside tile 1 -- every inner bound is 4096, the middle parts are empty, document 777 falls to part 0.
# [0, 2, 4]: the longest list ends in tile 3, the other tokens live in tiles 7 and 9 -- the last part takes all behind the last bound.
SPLIT_QUERIES = QUERIES + [[6, 3], [0, 2, 4]]
TOK, NT = pack_token_queries(SPLIT_QUERIES)
TILES = 10


@pytest.fixture(scope="module")
def split_index(hip):
    post, doc_len = text_corpus()
    idx = hip.HipIndex(4, hip.L2, hip.F32, capacity=N_IDS)
    idx.upload_rows(np.zeros((N_IDS, 4), dtype=np.float32), 1)
    idx.set_count(N_IDS)
    snap = snapshot_of(hip, post, doc_len, n_ids=N_IDS)
    idx.set_text(0, snap)
    ref = {name: [bm25_ref(post, doc_len, snap.total_docs, snap.avg_len, q, f) for q in SPLIT_QUERIES] for name, f in ALLOW.items()}
    yield idx, ref, {name: allow_bitmap(f) for name, f in ALLOW.items()}
    idx.close()


@pytest.mark.parametrize("allow", sorted(ALLOW))
@pytest.mark.parametrize("k", [1, 10, 1024])
@pytest.mark.parametrize("forced", [0, 2, 3, 10, 64])
def test_split_text_search(split_index, monkeypatch, forced, k, allow):
    idx, ref, bitmaps = split_index
    monkeypatch.setenv("KDB_TEXT_SPLIT", str(forced))
    parts, scratch, merge_lds, _ = idx.text_plan(0, NT.size, TOK.shape[1], k, 1)
    assert parts == (min(forced, TILES) if forced else 1) and scratch == (parts > 1) * -(-NT.size * parts * (12 * k + 8) // 8) * 8
    check_text_answer(idx.text_search(0, SPLIT_QUERIES, k, bitmaps[allow]), ref[allow], k)


def test_split_text_search_dev(split_index, monkeypatch):
    """the _dev form: a split call takes a lane and its scratch"""
    import torch
    idx, ref, _ = split_index
    monkeypatch.setenv("KDB_TEXT_SPLIT", "3")
    k, B = 10, NT.size
    assert idx.text_plan(0, B, TOK.shape[1], k)[0] == 3
    dev = lambda a: torch.from_numpy(a.view(np.int32)).cuda()
    ids, cnt, nc = (torch.zeros(s, dtype=torch.int32, device="cuda") for s in ((B, k), B, B))
    score, mx = (torch.zeros(s, dtype=torch.float64, device="cuda") for s in ((B, k), B))
    idx.text_search_dev(0, dev(TOK), dev(NT), k, ids, score, cnt, mx, nc)
    idx.sync()
    check_text_answer((ids.cpu().numpy().view(np.uint32), score.cpu().numpy(), cnt.cpu().numpy(), mx.cpu().numpy(), nc.cpu().numpy()), ref["none"], k)


def test_hybrid_search_split_equals_unsplit(hip, monkeypatch):
    """the text half of the hybrid call splits by the same plan: three tiles, KDB_TEXT_SPLIT=3 against 0, the very same arrays"""
    n, k = 10000, 20
    rng = np.random.default_rng(13)
    X = rng.standard_normal((n, HDIM)).astype(np.float32)
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    tokens = [[0, 1], [2], [1, 2, 0], [], [0], [1, 0]]
    Q = (X[rng.choice(n, len(tokens), replace=False)] + 0.05 * rng.standard_normal((len(tokens), HDIM))).astype(np.float32)
    post = {t: {int(d): TF[int(d) % 3] for d in rng.choice(np.arange(1, n + 1), m, replace=False)} for t, m in enumerate((3000, 700, 60))}
    idx = hip.HipIndex(HDIM, hip.COSINE, hip.F32, 16, 100, capacity=n)
    idx.upload_rows(X, 1)
    idx.build(n, batch=2048, ef_construction=100, seed=3)
    idx.set_text(0, snapshot_of(hip, post, {d: 5 + (d * 7) % 23 for d in range(1, n + 1)}, n_ids=n))
    out = {}
    for forced, parts in ((0, 1), (3, 3)):
        monkeypatch.setenv("KDB_TEXT_SPLIT", str(forced))
        assert idx.text_plan(0, len(tokens), 3, k, 1)[0] == parts
        out[forced] = [a.view(np.uint64 if a.dtype == np.float64 else a.dtype).tolist() for a in idx.hybrid_search(Q, k, 64, 0, tokens)]
    idx.close()
    assert min(out[0][2]) > 0 and out[0] == out[3]
