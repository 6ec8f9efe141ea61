"""Graph filters on the device (kdb_index_set_relations, kdb_graph_filter_eval[_dev]; graph_filter.hip) against the plain-Python
resolveGraphFilter of tests/graph_filter_ref.py.  Integer work: every list is compared word for word -- bit 0, the bits above count
and the padding words included (device outputs are pre-filled with 0xFF: a word nobody wrote shows) -- and every cardinality exactly."""
import numpy as np
import pytest

import graph_filter_ref as R
from kektordb_amd.index import GRAPH_QUERY_DTYPE

pytestmark = pytest.mark.gpu

RELS = [0, 5, 17, 40, 63]
MASKS = [2**64 - 1, 1 << 5, (1 << 0) | (1 << 63), (1 << 17) | (1 << 40) | 1, 0]
DEPTHS = [-1, 0, 1, 2, 3, 4, 5, 6, 99]
DIRS = [R.BOTH, R.OUT, R.IN, R.NONE]


def make(hip, edges, count, n_nodes):
    idx = hip.HipIndex(16, 0, 0, 8, 20, capacity=count + 5)
    idx.set_count(count)
    idx.set_relations(hip.RelationGraph(edges, n_nodes, {r: r for r in range(64)}))
    return idx


def queries(rows):
    return np.array([(root, depth, direction, 0, mask) for root, depth, direction, mask in rows], dtype=GRAPH_QUERY_DTYPE)


def run_dev(idx, q, words, d_and=None, and_of_query=None, stream=None, before=None):
    import torch
    d_lists = torch.full((q.size, words), -1, dtype=torch.int64, device="cuda")   # 0xFF in every byte
    d_card = torch.full((q.size,), 12345, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    if before:
        before()  # queued on `stream` in front of the call: nothing waits in between
    idx.graph_filter_dev(q, d_lists, d_card, d_and, and_of_query, stream=stream)
    torch.cuda.synchronize()
    return d_lists.cpu().numpy().view(np.uint64), d_card.cpu().numpy().view(np.uint32)


def same(got, want):
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (np.argwhere(got[0] != want[0])[:5], got[1], want[1])


def random_graph(count, seed=3):
    """count + 70 nodes, the last 70 ids the index does not hold: self loops, duplicate edges, cycles; node 2 has no edges"""
    rng = np.random.default_rng(seed)
    n = count + 70
    s, t, r = rng.integers(1, n + 1, 3 * n), rng.integers(1, n + 1, 3 * n), rng.choice(RELS, 3 * n)
    t[:20] = s[:20]
    edges = [(int(a), int(b), int(c)) for a, b, c in zip(s, r, t) if a != 2 and c != 2]
    return edges + edges[:50], n


def random_queries(count, n, B, seed=4):  # every direction x every mask; roots 0, isolated, above count, count, the last node, random
    roots = [0, 2, count + 1, count, n] + np.random.default_rng(seed).integers(1, n + 1, B).tolist()
    return queries([(roots[b], DEPTHS[b % 9], DIRS[b % 4], MASKS[(b // 4) % 5]) for b in range(B)])


@pytest.mark.parametrize("count", [63, 64, 65, 127, 128, 4097])
def test_random_multigraph(hip, count, monkeypatch):
    """B = 37 with mixed depths, directions and masks in one call and B = 1; words_per_list at the minimum and at minimum + 3; every
    KDB_GRAPH_PARTS gives the same bits, and so does a call cut into chunks of five queries; the host form, with and without lists"""
    edges, n = random_graph(count)
    idx = make(hip, edges, count, n)
    q = random_queries(count, n, 37)
    least = (n >> 6) + 1
    want = {w: R.lists_of(edges, count, q, w) for w in (least, least + 3)}
    for parts in ("0", "1", "2", "7", "512"):
        monkeypatch.setenv("KDB_GRAPH_PARTS", parts)
        for w in want:
            same(run_dev(idx, q, w), want[w])
    monkeypatch.setenv("KDB_GRAPH_SCRATCH_MAX", str(5 * 2 * least * 8))  # seven full chunks and one of two
    same(run_dev(idx, q, least), want[least])
    monkeypatch.delenv("KDB_GRAPH_SCRATCH_MAX")
    same(run_dev(idx, q[7:8], least), (want[least][0][7:8], want[least][1][7:8]))
    same(idx.graph_filter(q), want[least])
    lists, card = idx.graph_filter(q, want_lists=False)
    assert lists is None and np.array_equal(card, want[least][1])


def test_hubs_and_a_second_call_on_the_stream(hip, monkeypatch):
    """nodes 1..7: out-degree 16, 17, 64, 65, 256, 257, 5000; node 8: in-degree 5000; node 9 -> 100..399, each of out-degree 17: more
    heavy nodes in one sweep than the hub queue holds.  The second call finds the frontiers of the first in the lane's scratch."""
    import torch
    fan = lambda g, deg: [(g, g % 3, 1000 + (g * 7 + i * 13) % 5000) for i in range(deg)]
    edges = [e for g, deg in zip(range(1, 8), (16, 17, 64, 65, 256, 257, 5000)) for e in fan(g, deg)]
    edges += [(s, 1, 8) for s in range(1000, 6000)] + [(9, 2, t) for t in range(100, 400)] + [e for g in range(100, 400) for e in fan(g, 17)]
    count, words = 5500, (6000 >> 6) + 1  # nodes 5501..6000 are reached and never allowed
    idx = make(hip, edges, count, 6000)
    q = queries([(g, 1, R.OUT, 7) for g in range(1, 8)] + [(8, 2, R.IN, 7), (9, 3, R.OUT, 7), (1000, 3, R.BOTH, 7), (7, 2, R.BOTH, 2), (9, 2, R.OUT, 3)])
    want = R.lists_of(edges, count, q, words)
    st = torch.cuda.Stream()
    for parts in ("1", "3", "0"):
        monkeypatch.setenv("KDB_GRAPH_PARTS", parts)
        same(run_dev(idx, q, words, stream=st.cuda_stream), want)
        same(run_dev(idx, q, words, stream=st.cuda_stream), want)


def test_and_lists_join_a_filter_of_the_same_stream(hip):
    import torch
    count = 4097
    edges, n = random_graph(count)
    idx = make(hip, edges, count, n)
    x = (np.arange(1, count + 1) % 3).astype(np.float64)
    idx.set_column(0, 1, x, 1)
    term = lambda op, v: np.array([(op, 4, 0, 0, v)], dtype=hip.index.TERM_DTYPE)  # one F64 term, END_BLOCK
    q = random_queries(count, n, 37)
    words = (n >> 6) + 3
    and_of_query = np.array([(b % 3) - 1 for b in range(37)])  # -1 = NO_FILTER, 0, 1
    st = torch.cuda.Stream()
    d_and = torch.full((2, words), -1, dtype=torch.int64, device="cuda")
    flt = lambda: idx.filter_eval_dev([term(1, 0.0), term(4, 0.5)], d_and, None, stream=st.cuda_stream)  # x == 0, x > 0.5
    got = run_dev(idx, q, words, d_and, and_of_query, stream=st.cuda_stream, before=flt)
    and_lists = d_and.cpu().numpy().view(np.uint64)  # (the filter's own parity: test_gpu_filter_eval.py)
    assert [int(np.unpackbits(l.view(np.uint8)).sum()) for l in and_lists] == [count // 3, count - count // 3]
    want = R.lists_of(edges, count, q, words, and_lists, and_of_query)
    same(got, want)
    same(idx.graph_filter(q, words, and_lists=and_lists, and_of_query=and_of_query), want)


def test_chain_snapshot_lifecycle_and_refusals(hip):
    edges = [(g, 0, g + 1) for g in range(1, 8)]
    idx = hip.HipIndex(16, 0, 0, 8, 20, capacity=200)
    idx.set_count(100)
    q = queries([(1, 5, R.OUT, 1)])
    assert idx.relations_info() == (0, 0, 0)
    with pytest.raises(hip.KdbError, match="no relation snapshot"):
        idx.graph_filter(q, 2)
    idx.set_relations(hip.RelationGraph(edges, 8))
    assert idx.relations_info()[:2] == (8, 7) and idx.relations_info()[2] > 0
    same(idx.graph_filter(q), R.lists_of(edges, 100, q, 2))  # words follow max(count, n_nodes)
    qc = queries([(1, d, R.OUT, 1) for d in (-1, 0, 1, 4, 5, 6, 99)] + [(8, 3, R.IN, 1), (4, 2, R.BOTH, 1), (4, 2, R.NONE, 1), (4, 2, R.OUT, 2)])
    same(run_dev(idx, qc, 2), R.lists_of(edges, 100, qc, 2))  # the chain pins the depth clamp: the reference's own cardinalities
    assert R.lists_of(edges, 100, qc, 2)[1].tolist() == [2, 2, 2, 5, 6, 6, 6, 4, 5, 1, 1]
    refused = [(lambda: idx.graph_filter(q, 1), "words_per_list"), (lambda: idx.graph_filter(queries([(9, 1, R.OUT, 1)])), "root above"),
               (lambda: idx.graph_filter(queries([(1, 1, 4, 1)])), "direction"),
               (lambda: idx.graph_filter(q, and_lists=np.zeros((1, 2), dtype=np.uint64), and_of_query=[1]), "names no list")]
    for call, word in refused:
        with pytest.raises(hip.KdbError, match=word):
            call()
    edges2 = [(300, 1, 1), (1, 1, 300), (300, 1, 7)]  # replaced wholesale: more nodes than the index has capacity for
    idx.set_relations(hip.RelationGraph(edges2, 300, {0: 0, 1: 1}))
    assert idx.relations_info()[:2] == (300, 3)
    q2 = queries([(1, 2, R.OUT, 2), (1, 5, R.OUT, 1)])
    same(idx.graph_filter(q2), R.lists_of(edges2, 100, q2, 5))
    idx.drop_relations()
    assert idx.relations_info() == (0, 0, 0)
