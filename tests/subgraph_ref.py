"""Engine.VExtractSubgraph (pkg/engine/graph.go:296-386) in plain Python over graph node numbers, queue and edges-before-visited as written;
the gate: ComputeDistanceToVector (hnsw_index.go:3381-3468) in numpy float64 from the stored rows, 999999.0 for a node that is not live."""
from collections import deque

import numpy as np

from test_gpu_compress_edges import np_quantize as quantize  # Quantizer.Quantize (quantizer.go:150-176)

NOT_LIVE, F16, I8 = 999999.0, 1, 2


def distances(rows, live, guide, metric, precision, norms=None, absmax=0.0):
    """dist(t) as float64 for every graph node t < live.size; rows [count + 1, dim] in stored form, live: found by GetNodeData"""
    d = np.full(live.size, NOT_LIVE)
    ids = np.flatnonzero(live)
    g = np.asarray(guide, np.float32)
    if precision == I8:  # :3436-3464 -- the guide quantised without normalising, an exact dot, the query norm rounded to float32
        q = quantize(g, absmax).astype(np.int64)
        qn = np.float64(np.float32(np.sqrt(np.float64((q * q).sum()))) or 1)
        sn = norms[ids].astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            sim = np.clip((rows[ids].astype(np.int64) @ q).astype(np.float64) / (qn * sn), -1.0, 1.0)
        d[ids] = np.where(sn == 0, 1.0, 1.0 - sim)
        return d
    g = (g.astype(np.float16) if precision == F16 else g).astype(np.float64)
    x = rows[ids].astype(np.float64)  # (float16 rows: the stored halves widened)
    d[ids] = 1.0 - x @ (g / np.sqrt(g @ g)) if metric == 1 else ((x - g) ** 2).sum(axis=1)
    return d


def extract(out, inn, root, max_depth, rel_mask, passes=None):
    """(node set, edge records (src, dst, info)) of one query; passes: None (no guide) or a bool per graph node"""
    if root == 0:
        return set(), []
    max_depth = 1 if max_depth <= 0 else 5 if max_depth > 5 else max_depth
    visited, edges, queue = {root}, [], deque([(root, 0)])
    while queue:
        node, depth = queue.popleft()
        if depth >= max_depth:
            continue
        for direction, lists in ((0, out), (1, inn)):
            for r, t in lists.get(node, ()):
                if not (rel_mask >> r) & 1 or (passes is not None and not passes[t]):
                    continue
                edges.append((t, node, r | 256 | depth << 16) if direction else (node, t, r | depth << 16))  # before `visited` is looked at
                if t not in visited:
                    visited.add(t)
                    queue.append((t, depth + 1))
    return visited, edges


def results(edges, queries, words, dist_of_query=None):
    """(nodes [B, words], n_nodes [B], n_edges [B], [sorted (n, 3) records]); dist_of_query[b]: float64 per graph node, for guided queries"""
    out, inn = {}, {}
    for s, r, t in edges:
        out.setdefault(int(s), []).append((int(r), int(t)))
        inn.setdefault(int(t), []).append((int(r), int(s)))
    nodes, recs, n_nodes = np.zeros((len(queries), words), dtype=np.uint64), [], []
    for b, q in enumerate(queries):
        passes = dist_of_query[b] <= float(q[5]) if int(q[2]) & 1 else None
        vs, es = extract(out, inn, int(q[0]), int(q[1]), int(q[4]), passes)
        for i in vs:
            nodes[b, i >> 6] |= np.uint64(1 << (i & 63))
        n_nodes.append(len(vs))
        recs.append(np.array(sorted(es), dtype=np.uint32).reshape(-1, 3))
    return nodes, np.array(n_nodes, dtype=np.uint32), np.array([len(e) for e in recs], dtype=np.uint32), recs
