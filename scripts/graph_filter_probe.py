"""Graph filters on a synthetic relation graph: --nodes graph nodes (1M, 10M), out-degrees from a Zipf law cut at 1000 (mean about 8),
--hubs nodes of --hub-degree out-edges (150k) on top, uniform targets, 4 relations; count = nodes (every node is an internal id).

  leg 1  kdb_graph_filter_eval_dev on device buffers, direction BOTH, every relation: depth 1 / 3 / 5 x B = 1 / 64 / 1024;
  leg 2  the same queries through `host_bfs`: resolveGraphFilter restated in numpy on the host (level by level over the CSR, a bool
         array as visited set, packed to words) plus the host-to-device copy of the lists.  It stands for the host path the call
         replaces; it is NOT the Go binary (no maps, no string ids, no GC).  At most --host-queries queries per round: ms per query;
  leg 3  B = 1, depth 3, KDB_GRAPH_PARTS forced to 1 ... 512 (what KDB_GRAPH_MIN_WORDS_PER_PART has to justify).

The legs ALTERNATE in one process, --reps (31) times after --warmup rounds; medians, and the spread as (min, max).  Before anything is
timed the device lists must equal host_bfs word for word on the first queries.  Reported per device cell: ms per call; the words
the launches sweep (init and finish over the lists, one frontier per level) per second beside the streaming ceiling kdb_probe_stream
measures in the same run; edges expanded per second, the edges counted by host_bfs on the sampled queries.  The library in use is
recorded: KDB_GRAPH_LIGHT_DEG is a build constant, its 8 / 32 legs are other builds given through KEKTOR_HIP_LIB.

usage: python scripts/graph_filter_probe.py [--nodes N] [--out profiles/graph_filter_probe.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def log(*a):
    print("[graph_filter_probe]", *a, file=sys.stderr, flush=True)


def ms(x, per=1):
    x = np.asarray(x) * 1e3 / per
    return {"median_ms": round(float(np.median(x)), 5), "min_ms": round(float(x.min()), 5), "max_ms": round(float(x.max()), 5)}


def make_graph(a, rng):
    deg = np.minimum(rng.zipf(a.zipf, a.nodes + 1), 1000).astype(np.int64)
    deg[0] = 0
    deg[rng.choice(np.arange(1, a.nodes + 1), a.hubs, replace=False)] = a.hub_degree
    off = np.zeros(a.nodes + 2, dtype=np.uint64)
    off[1:] = np.cumsum(deg)
    E = int(off[-1])
    return off, rng.integers(1, a.nodes + 1, E, dtype=np.uint32), rng.integers(0, 4, E).astype(np.uint8)


def transpose(off, dst, rel, n):
    order = np.argsort(dst, kind="stable")
    src = np.repeat(np.arange(n + 1, dtype=np.uint32), np.diff(off.astype(np.int64)))
    t_off = np.zeros(n + 2, dtype=np.uint64)
    t_off[1:] = np.cumsum(np.bincount(dst, minlength=n + 1))
    return t_off, src[order], rel[order]


def host_bfs(csr, n, root, depth, mask, words):
    """(list words, edges expanded) of one query, direction BOTH"""
    visited = np.zeros(words * 64, dtype=bool)
    visited[root] = True
    frontier, edges = np.array([root], dtype=np.int64), 0
    for _ in range(min(max(depth, 1), 5)):
        found = []
        for off, dst, rel in csr:
            lo, cnt = off[frontier].astype(np.int64), (off[frontier + 1] - off[frontier]).astype(np.int64)
            at = np.repeat(lo - (np.cumsum(cnt) - cnt), cnt) + np.arange(int(cnt.sum()))
            edges += at.size
            found.append(dst[at][((mask >> rel[at].astype(np.uint64)) & np.uint64(1)).astype(bool)])
        t = np.unique(np.concatenate(found))
        frontier = t[~visited[t]].astype(np.int64)
        visited[frontier] = True
        if not frontier.size:
            break
    return np.packbits(visited, bitorder="little").view(np.uint64), edges


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=1_000_000)
    ap.add_argument("--zipf", type=float, default=1.8)
    ap.add_argument("--hubs", type=int, default=4)
    ap.add_argument("--hub-degree", type=int, default=150_000)
    ap.add_argument("--reps", type=int, default=31)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-queries", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "graph_filter_probe.json"))
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "graph_filter_probe needs a GPU"
    import kektordb_amd as K
    from kektordb_amd.index import GRAPH_QUERY_DTYPE, GDIR_BOTH, RelationGraph
    rng = np.random.default_rng(7)
    n = a.nodes
    off, dst, rel = make_graph(a, rng)
    csr = [(off, dst, rel), transpose(off, dst, rel, n)]
    log(f"{n} nodes, {dst.size} edges (mean out-degree {dst.size / n:.2f}), largest {int(np.diff(off.astype(np.int64)).max())}")
    idx = K.HipIndex(16, K.L2, K.F32, capacity=n)
    idx.upload_rows(np.zeros((n, 16), dtype=np.float32), 1)
    idx.set_count(n)
    idx.set_relations(RelationGraph.from_arrays(off, dst, rel))
    ceiling = idx.probe_stream()
    words, wpn, mask = (n >> 6) + 1, (n >> 6) + 1, np.uint64(15)
    roots = rng.integers(1, n + 1, 1024)
    make_q = lambda B, depth: np.array([(int(r), depth, GDIR_BOTH, 0, 15) for r in roots[:B]], dtype=GRAPH_QUERY_DTYPE)
    d_lists = torch.zeros((1024, words), dtype=torch.int64, device="cuda")
    d_card = torch.zeros(1024, dtype=torch.int32, device="cuda")
    pinned = torch.zeros((a.host_queries, words), dtype=torch.int64).pin_memory()

    def device_call(q):
        t0 = time.perf_counter()
        idx.graph_filter_dev(q, d_lists[:q.size], d_card[:q.size])
        idx.sync()
        return time.perf_counter() - t0

    def host_call(q):
        t0 = time.perf_counter()
        edges = 0
        for b in range(q.size):
            lst, e = host_bfs(csr, n, int(q["root"][b]), int(q["max_depth"][b]), mask, words)
            pinned[b].numpy().view(np.uint64)[:] = lst[:words]
            edges += e
        d_lists[:q.size].copy_(pinned[:q.size], non_blocking=True)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, edges

    result = {"nodes": n, "edges": int(dst.size), "library": K.LIB_PATH, "stream_GBps": round(ceiling, 1), "cells": [], "parts": []}
    for depth in (1, 3, 5):
        qh = make_q(a.host_queries, depth)
        host_call(qh)
        want = d_lists[:qh.size].cpu().numpy().copy()
        device_call(qh)
        assert np.array_equal(d_lists[:qh.size].cpu().numpy(), want), f"depth {depth}: the device lists differ from host_bfs"
        for B in (1, 64, 1024):
            q = make_q(B, depth)
            t_dev, t_host, edges = [], [], 0
            for r in range(a.warmup + a.reps):  # the legs alternate
                td, (th, edges) = device_call(q), host_call(qh)
                if r >= a.warmup:
                    t_dev.append(td)
                    t_host.append(th)
            swept = B * 8 * (3 * words + 2 * wpn + depth * wpn)  # init writes lists and both frontiers, each level reads one, finish reads and writes the lists
            med = float(np.median(t_dev))
            cell = {"depth": depth, "B": B, "device": ms(t_dev), "host_per_query": ms(t_host, a.host_queries), "swept_GBps": round(swept / med / 1e9, 1),
                    "share_of_stream": round(swept / med / 1e9 / ceiling, 3), "edges_per_query_sampled": edges // a.host_queries,
                    "edges_per_s_est": round(edges / a.host_queries * B / med)}
            log(cell)
            result["cells"].append(cell)
    q = make_q(1, 3)
    times = {p: [] for p in (1, 4, 16, 61, 128, 512)}
    for r in range(a.warmup + a.reps):
        for p in times:
            os.environ["KDB_GRAPH_PARTS"] = str(p)
            t = device_call(q)
            if r >= a.warmup:
                times[p].append(t)
    os.environ.pop("KDB_GRAPH_PARTS")
    result["parts"] = [{"parts": p, **ms(t)} for p, t in times.items()]
    log(result["parts"])
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    idx.close()


if __name__ == "__main__":
    main()
