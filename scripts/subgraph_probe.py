"""Subgraph extraction on a synthetic relation graph: --nodes graph nodes, out-degrees from a Zipf law cut at 1000 (mean about 8),
--hubs nodes of --hub-degree out-edges on top, uniform targets, 4 relations; count = nodes, float32 cosine rows of --dim columns.

  leg 1  kdb_subgraph_extract_dev on device buffers, every relation, depth 2 / 3 x B = 1 / 16 / 64, unguided and guided (threshold at
         the median distance of the first query's guide, so about half the far ends pass);
  leg 2  the same queries through `host_extract`: VExtractSubgraph restated in plain Python on the host over the same snapshot
         (the loop of tests/subgraph_ref.py over the CSR arrays), its gate one numpy float64 distance per EDGE as shouldTraverse
         computes it (no cache, like the reference).  It stands for the host path the call replaces; it is NOT the Go binary.  At
         most --host-queries queries per round: ms per query.

The legs ALTERNATE in one process, --reps times after --warmup rounds; medians, and the spread as (min, max).  Before anything is
timed the device result must equal the restatement on the sampled queries: node bitmaps word for word, edge counts exactly.
Reported per cell: ms per call, edges found per second, and the distances the restatement computed per sampled query.

usage: python scripts/subgraph_probe.py [--nodes N] [--out profiles/subgraph_probe.json]"""
import argparse
import json
import os
import sys
import time
from collections import deque

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def log(*a):
    print("[subgraph_probe]", *a, file=sys.stderr, flush=True)


def ms(x, per=1):
    x = np.asarray(x) * 1e3 / per
    return {"median_ms": round(float(np.median(x)), 5), "min_ms": round(float(x.min()), 5), "max_ms": round(float(x.max()), 5)}


def host_extract(csr, rows, root, depth, mask, guide, threshold):
    """(node set, edges found, distances computed) of one query: subgraph_ref.extract's loop over the CSR arrays, the gate per edge"""
    g = None if guide is None else guide.astype(np.float64) / np.sqrt(float(guide.astype(np.float64) @ guide.astype(np.float64)))
    visited, n_edges, n_dist, queue = {root}, 0, 0, deque([(root, 0)])
    while queue:
        node, d = queue.popleft()
        if d >= depth:
            continue
        for off, dst, rel in csr:
            for e in range(int(off[node]), int(off[node + 1])):
                t = int(dst[e])
                if not (mask >> int(rel[e])) & 1:
                    continue
                if g is not None:
                    n_dist += 1
                    if not 1.0 - float(rows[t].astype(np.float64) @ g) <= threshold:
                        continue
                n_edges += 1
                if t not in visited:
                    visited.add(t)
                    queue.append((t, d + 1))
    return visited, n_edges, n_dist


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=200_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--zipf", type=float, default=1.8)
    ap.add_argument("--hubs", type=int, default=4)
    ap.add_argument("--hub-degree", type=int, default=20_000)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-queries", type=int, default=2)
    ap.add_argument("--edge-cap", type=int, default=1 << 16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "subgraph_probe.json"))
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "subgraph_probe needs a GPU"
    import kektordb_amd as K
    from kektordb_amd.index import SUBGRAPH_QUERY_DTYPE, RelationGraph
    from graph_filter_probe import make_graph, transpose
    rng = np.random.default_rng(7)
    n = a.nodes
    off, dst, rel = make_graph(a, rng)
    csr = [(off, dst, rel), transpose(off, dst, rel, n)]
    rows = np.zeros((n + 1, a.dim), dtype=np.float32)
    rows[1:] = rng.standard_normal((n, 8), dtype=np.float32) @ rng.standard_normal((8, a.dim), dtype=np.float32)
    rows[1:] /= np.linalg.norm(rows[1:], axis=1, keepdims=True)
    idx = K.HipIndex(a.dim, K.COSINE, K.F32, capacity=n)
    idx.upload_rows(rows[1:], 1)
    idx.set_count(n)
    idx.set_relations(RelationGraph.from_arrays(off, dst, rel))
    log(f"{n} nodes, {dst.size} edges, rows of {a.dim} columns")
    words = (n >> 6) + 1
    roots = rng.integers(1, n + 1, 64)
    guides = rows[rng.integers(1, n + 1, 64)] + 0.02 * rng.standard_normal((64, a.dim)).astype(np.float32)
    threshold = float(np.median(1.0 - rows[1:].astype(np.float64) @ (guides[0] / np.linalg.norm(guides[0])).astype(np.float64)))
    d_nodes = torch.zeros((64, words), dtype=torch.int64, device="cuda")
    d_nn, d_ne = torch.zeros(64, dtype=torch.int32, device="cuda"), torch.zeros(64, dtype=torch.int32, device="cuda")
    d_edges = torch.zeros((64, a.edge_cap, 3), dtype=torch.int32, device="cuda")
    d_guides = torch.from_numpy(guides).cuda()

    def make_q(B, depth, guided):
        return np.array([(int(r), depth, 1 if guided else 0, 0, 15, threshold if guided else 0.0) for r in roots[:B]], dtype=SUBGRAPH_QUERY_DTYPE)

    def device_call(q):
        t0 = time.perf_counter()
        idx.extract_subgraph_dev(q, d_nodes[:q.size], d_nn[:q.size], d_ne[:q.size], d_edges[:q.size], d_guides[:q.size])
        idx.sync()
        return time.perf_counter() - t0

    def host_call(q):
        t0 = time.perf_counter()
        out = [host_extract(csr, rows, int(r["root"]), int(r["max_depth"]), 15, guides[b] if r["flags"] else None, threshold) for b, r in enumerate(q)]
        return time.perf_counter() - t0, out

    result = {"nodes": n, "edges": int(dst.size), "dim": a.dim, "library": K.LIB_PATH, "threshold": threshold, "cells": []}
    for guided in (False, True):
        for depth in (2, 3):
            qh = make_q(a.host_queries, depth, guided)
            _, want = host_call(qh)
            device_call(qh)
            got_nodes, got_ne = d_nodes[:qh.size].cpu().numpy().view(np.uint64), d_ne[:qh.size].cpu().numpy()
            for b, (vs, ne, _) in enumerate(want):
                bits = np.flatnonzero(np.unpackbits(got_nodes[b].view(np.uint8), bitorder="little")).tolist()
                assert bits == sorted(vs) and int(got_ne[b]) == ne, f"depth {depth} guided {guided} query {b}: the device result differs from the restatement"
            for B in (1, 16, 64):
                q = make_q(B, depth, guided)
                t_dev, t_host = [], []
                for r in range(a.warmup + a.reps):  # the legs alternate
                    td, (th, _) = device_call(q), host_call(qh)
                    if r >= a.warmup:
                        t_dev.append(td)
                        t_host.append(th)
                med, edges = float(np.median(t_dev)), int(d_ne[:B].cpu().numpy().astype(np.int64).sum())
                cell = {"guided": guided, "depth": depth, "B": B, "device": ms(t_dev), "host_per_query": ms(t_host, a.host_queries), "edges_found": edges,
                        "edges_per_s": round(edges / med), "host_distances_per_query_sampled": sum(w[2] for w in want) // a.host_queries}
                log(cell)
                result["cells"].append(cell)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    idx.close()


if __name__ == "__main__":
    main()
