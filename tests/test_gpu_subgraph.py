"""kdb_subgraph_extract[_dev] against tests/subgraph_ref.py: bitmaps word for word (outputs pre-filled with 0xFF), counts exactly, records sorted.
Guided float32 / float16 thresholds keep 1e-4 relative (the bound between accumulation orders) from every live distance; int8 is exact."""
import numpy as np
import pytest

import graph_filter_ref as GR
import subgraph_ref as R
from kektordb_amd.index import GRAPH_QUERY_DTYPE, SUBGRAPH_QUERY_DTYPE
from test_gpu_graph_filter import DEPTHS, MASKS, random_graph

pytestmark = pytest.mark.gpu
ALL = 2**64 - 1


def make(hip, edges, count, n_nodes, dim=16, metric=0, precision=0, deleted=()):
    """(index, or None without hip; stored rows; live mask over graph nodes; norms; absmax); rows of effective dimension 4: distances spread"""
    rng = np.random.default_rng(5)
    x = (rng.standard_normal((count, 4)) @ rng.standard_normal((4, dim))).astype(np.float32)
    if metric == 1 and precision == 0:
        x /= np.linalg.norm(x, axis=1, keepdims=True)
    absmax = float(np.abs(x).max())
    rows = np.zeros((count + 1, dim), dtype=(np.float32, np.float16, np.int8)[precision])
    rows[1:] = R.quantize(x, absmax) if precision == 2 else x
    norms = np.sqrt((rows.astype(np.int64) ** 2).sum(axis=1).astype(np.float64)).astype(np.float32)
    live = (np.arange(n_nodes + 1) - 1) % 2**32 < count  # ids 1..count
    live[list(deleted)] = False
    if hip is None:
        return None, rows, live, norms, absmax
    idx = hip.HipIndex(dim, metric, precision, 8, 20, capacity=count + 5)
    idx.upload_rows(rows[1:].view(np.uint16) if precision == 1 else rows[1:], 1)  # (halves travel as their bits)
    if precision == 2:
        idx.upload_norms(norms[1:], 1)
        idx.set_quantizer(absmax)
    idx.set_count(count)
    if len(deleted):
        idx.Delete(list(deleted))
    idx.set_relations(hip.RelationGraph(edges, n_nodes, {r: r for r in range(64)}))
    return idx, rows, live, norms, absmax


def queries(rows):
    return np.array([(root, depth, 0 if thr is None else 1, 0, mask, 0.0 if thr is None else thr) for root, depth, mask, thr in rows], dtype=SUBGRAPH_QUERY_DTYPE)


def run_dev(idx, q, words, cap, guides=None, stream=None):
    import torch
    full = lambda shape, dtype=torch.int32: torch.full(shape, -1, dtype=dtype, device="cuda")  # 0xFF in every byte
    d_nodes, d_nn, d_ne, d_edges = full((q.size, words), torch.int64), full((q.size,)), full((q.size,)), full((q.size, cap, 3)) if cap else None
    d_g = None if guides is None else torch.from_numpy(np.ascontiguousarray(guides, dtype=np.float32)).cuda()
    torch.cuda.synchronize()
    idx.extract_subgraph_dev(q, d_nodes, d_nn, d_ne, d_edges, d_g, stream=stream)
    torch.cuda.synchronize()
    edges = np.zeros((q.size, 0, 3), np.uint32) if d_edges is None else d_edges.cpu().numpy().view(np.uint32)
    return d_nodes.cpu().numpy().view(np.uint64), d_nn.cpu().numpy().view(np.uint32), d_ne.cpu().numpy().view(np.uint32), edges


def same(got, want, records=True):
    assert np.array_equal(got[0], want[0]), np.argwhere(got[0] != want[0])[:5]
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), (got[1], want[1], got[2], want[2])
    for b, rec in enumerate(want[3] if records else ()):
        e = np.asarray(got[3]).view(np.uint32).reshape(len(want[3]), -1, 3)[b, :len(rec)]
        assert np.array_equal(e[np.lexsort(e.T[::-1])], rec), b


@pytest.mark.parametrize("count", [63, 64, 65, 4097])
def test_unguided_random_multigraph(hip, count, monkeypatch):
    """B = 37 (mixed depths and masks, root 0, an empty mask) and B = 1; forced parts; chunks of five; resolveGraphFilter's nodes"""
    edges, n = random_graph(count)
    idx = make(hip, edges, count, n)[0]
    roots = [0, 2, count + 1, count, n] + np.random.default_rng(4).integers(1, n + 1, 37).tolist()
    q = queries([(roots[b], DEPTHS[b % 9], MASKS[(b // 4) % 5], None) for b in range(37)])
    words = (n >> 6) + 1
    want = R.results(edges, q, words)
    cap = int(want[2].max())
    held = np.packbits((np.arange(words * 64) - 1) % 2**32 < count, bitorder="little").view(np.uint64)  # ids 1..count
    gq = np.array([(r[0], r[1], GR.BOTH, 0, r[4]) for r in q], dtype=GRAPH_QUERY_DTYPE)
    assert np.array_equal(want[0] & held, GR.lists_of(edges, count, gq, words)[0])
    for parts in ("1", "7", "512", "0"):
        monkeypatch.setenv("KDB_GRAPH_PARTS", parts)
        same(run_dev(idx, q, words, cap), want)
    monkeypatch.setenv("KDB_GRAPH_SCRATCH_MAX", str(5 * 5 * words * 8))  # seven full chunks and one of two
    same(run_dev(idx, q, words + 3, cap), R.results(edges, q, words + 3))
    monkeypatch.delenv("KDB_GRAPH_SCRATCH_MAX")
    same(run_dev(idx, q[7:8], words, cap), tuple(w[7:8] for w in want))


def threshold(live_dist, frac):
    """the middle of the widest of the 16 gaps around a quantile of the live distances; the margin is a condition on the INPUTS"""
    ds = np.sort(live_dist)
    i = int(frac * ds.size)
    j = i - 8 + int(np.argmax(np.diff(ds[i - 8:i + 9])))
    thr = float(ds[j] + ds[j + 1]) / 2
    assert np.abs(ds - thr).min() > 1e-4 * abs(thr), (frac, thr)
    return thr


@pytest.mark.parametrize("precision,metric,dim", [(0, 1, 16), (0, 0, 100), (0, 1, 768), (1, 0, 100), (2, 1, 100)])
def test_guided(hip, precision, metric, dim):
    """thresholds near the 10th, 50th, 90th percentile and at 1e6 (not-live nodes pass); int8, query 0: EQUAL to a far end's distance, pins <="""
    count, B = 4097, 8
    edges, n = random_graph(count)
    deleted, words = range(5, count, 9), (n >> 6) + 1
    _, rows, live, norms, absmax = make(None, edges, count, n, dim, metric, precision, deleted)
    rng = np.random.default_rng(9)
    base = rows[rng.integers(1, count + 1, B)].astype(np.float32) * (absmax / 127 if precision == 2 else 1)
    guides = (base + 0.3 * np.abs(base).mean() * rng.standard_normal((B, dim))).astype(np.float32)  # a stored row, blurred
    dist = [R.distances(rows, live, guides[b], metric, precision, norms, absmax) for b in range(B)]
    thr = lambda b, frac: float(np.sort(dist[b][live])[int(frac * live.sum())]) if precision == 2 else threshold(dist[b][live], frac)
    rows_q = [(int(rng.integers(1, n + 1)), 2 + b % 4, MASKS[(0, 0, 3, 2)[b % 4]], 1e6 if b % 4 == 3 else thr(b, (0.1, 0.5, 0.9)[b % 4])) for b in range(B)]
    if precision == 2:
        root, t = next((s, t) for s, r, t in edges if s != t and live[t])
        rows_q[0] = (root, 1, ALL, float(dist[0][t]))
    q = queries(rows_q)
    want = R.results(edges, q, words, dist)
    if precision == 2:
        strict = R.results(edges, q[:1], words, [np.where(dist[0] == q[0][5], np.inf, dist[0])])
        assert strict[1][0] < want[1][0] and strict[2][0] < want[2][0]
    idx = make(hip, edges, count, n, dim, metric, precision, deleted)[0]
    same(run_dev(idx, q, words, int(want[2].max()), guides), want)


def test_guided_f32_boundary(hip, oracle):
    """100 columns: the threshold is the oracle's GPU-order distance of a far end of the root; the next float64 below keeps it out"""
    count, dim = 300, 100
    edges, n = random_graph(count)
    idx, rows, live, _, _ = make(hip, edges, count, n, dim, 1, 0)
    orc = oracle.OracleIndex(dim, oracle.COSINE, oracle.F32, 8, 20)
    orc.add_many(rows[1:])
    orc.set_arith(oracle.ARITH_HIP_WAVE)
    rows = orc.rows()  # (Add normalises once more: the oracle's rows are the stored ones)
    idx.upload_rows(rows[1:], 1)
    guide = (rows[7] + 0.3 * np.random.default_rng(1).standard_normal(dim)).astype(np.float32)
    root, t = next((s, t) for s, r, t in edges if s != t and t <= count)
    dist = np.full(n + 1, R.NOT_LIVE)
    dist[1:count + 1] = orc.distances(guide, np.arange(1, count + 1, dtype=np.uint32))
    for thr in (float(dist[t]), float(np.nextafter(dist[t], -np.inf))):
        q = queries([(root, 1, ALL, thr)])
        want = R.results(edges, q, (n >> 6) + 1, [dist])
        assert bool((want[0][0, t >> 6] >> np.uint64(t & 63)) & np.uint64(1)) == (thr == dist[t])
        same(run_dev(idx, q, (n >> 6) + 1, 64, guide[None]), want)


def test_hubs_and_a_second_call_on_the_stream(hip):
    """more heavy nodes in a sweep than the hub queue holds, more candidates in a level than a gate batch; the second call finds bitmaps"""
    import torch
    fan = lambda g, deg: [(g, g % 3, 1000 + (g * 7 + i * 13) % 5000) for i in range(deg)]
    edges = [e for g, deg in zip(range(1, 8), (16, 17, 64, 65, 256, 257, 5000)) for e in fan(g, deg)]
    edges += [(s, 1, 8) for s in range(1000, 6000)] + [(9, 2, t) for t in range(100, 400)] + [e for g in range(100, 400) for e in fan(g, 17)]
    count, n = 5500, 6000
    idx, rows, live, _, _ = make(hip, edges, count, n, deleted=range(1003, 5000, 7))
    guide = rows[1234] + 0.5
    dist = R.distances(rows, live, guide, 0, 0)
    roots = [(g, 1) for g in range(1, 8)] + [(8, 2), (9, 3), (1000, 3), (7, 2), (9, 2)]
    q = queries([(g, d, 7, t) for g, d in roots for t in (None, threshold(dist[live], 0.5), 1e6)])
    want = R.results(edges, q, (n >> 6) + 1, [dist] * q.size)
    st = torch.cuda.Stream()
    for _ in range(2):
        same(run_dev(idx, q, (n >> 6) + 1, int(want[2].max()), np.tile(guide, (q.size, 1)), stream=st.cuda_stream), want)


def test_hub_queue_fills_in_the_second_direction(hip, monkeypatch):
    """root 1 -> 400 consecutive middle nodes, each light outwards (1..16 edges) and heavy inwards (18 distinct sources): with one
    workgroup the hub queue fills while a word's in-edges are queued, after that word's out-edges were visited by their lanes.  A sweep
    that took such a word up again at the first direction would write those records twice: n_edges and the sorted records show it."""
    import test_gpu_graph_filter as F
    hub_cap, light = 256, 16  # KDB_GRAPH_HUB_CAP, KDB_GRAPH_LIGHT_DEG (kdb_graph_plan.h)
    middle, count, n = range(100, 500), 2000, 2000
    edges = [(1, 0, m) for m in middle]
    edges += [(m, 1, 600 + (m * 5 + i * 3) % 1400) for m in middle for i in range(1 + m % 16)]
    edges += [(600 + (m * 17 + i) % 1400, 2, m) for m in middle for i in range(17)]
    outs, ins = {}, {}
    for s, _, t in edges:
        outs.setdefault(s, set()).add(t)
        ins.setdefault(t, set()).add(s)
    level1 = outs[1] | ins.get(1, set())
    assert sum(1 <= len(outs.get(m, ())) <= light and len(ins[m]) > light for m in level1) > hub_cap + 64
    idx, rows, live, _, _ = make(hip, edges, count, n)
    words = (n >> 6) + 1
    q = queries([(1, 2, 7, None), (1, 2, 7, 1e6)])
    guides = np.tile(rows[7] + 0.5, (2, 1))
    want = R.results(edges, q, words, [R.distances(rows, live, guides[0], 0, 0)] * 2)
    assert want[2][0] == want[2][1] == len(edges) + len(middle)  # every edge once, the root's also from their far ends
    gq = F.queries([(1, 2, GR.BOTH, 7)])
    monkeypatch.setenv("KDB_GRAPH_PARTS", "1")
    same(run_dev(idx, q, words, int(want[2][0]), guides), want)
    F.same(F.run_dev(idx, gq, words), GR.lists_of(edges, count, gq, words))


def test_edge_cap_and_the_host_form(hip):
    count = 128
    edges, n = random_graph(count)
    idx, rows, live, _, _ = make(hip, edges, count, n)
    dist = R.distances(rows, live, rows[3], 0, 0)
    q = queries([(1, 3, ALL, None), (1, 3, ALL, threshold(dist[live], 0.8)), (count + 1, 5, 1 << 5, None)])
    guides, words = np.tile(rows[3], (3, 1)), (n >> 6) + 1
    want = R.results(edges, q, words, [dist] * 3)
    most = int(want[2].max())
    assert most > 40 and 0 < want[2][1] < want[2][0]
    same(run_dev(idx, q, words, most, guides), want)  # a cap equal to the count
    same(idx.extract_subgraph(q, guides, most), want)  # the host form
    same(run_dev(idx, q, words, 0, guides), want, records=False)  # counts only; below: a cap under the count, members only
    for got in (run_dev(idx, q, words, 40, guides), idx.extract_subgraph(q, guides, 40)):
        same(got, want, records=False)
        assert all(e in pool.tolist() for b, pool in enumerate(want[3]) for e in got[3].view(np.uint32).reshape(3, 40, 3)[b, :min(40, len(pool))].tolist())


def test_refusals_and_empties(hip):
    edges = [(g, 0, g + 1) for g in range(1, 8)]
    idx = hip.HipIndex(16, 0, 0, 8, 20, capacity=200)
    idx.set_count(100)
    with pytest.raises(hip.KdbError, match="no relation snapshot"):
        idx.extract_subgraph(queries([(1, 5, 1, None)]), words_per_list=2)
    idx.set_relations(hip.RelationGraph(edges, 64))
    for q, words, word in [((65, 1, 1, None), 0, "root above"), ((1, 1, 1, 0.5), 0, "null guides"), ((1, 5, 1, None), 1, "words_per_list")]:
        with pytest.raises(hip.KdbError, match=word):
            idx.extract_subgraph(queries([q]), words_per_list=words)
    q = queries([(0, 3, 1, None), (3, 3, 0, None), (3, 1, 1, None)])  # root 0: empty; an empty mask: the root alone; the chain's neighbours
    same(run_dev(idx, q, 2, 4), R.results(edges, q, 2))
