"""kdb_index_vacuum on the headline corpus (1M x 768 cosine, clustered, efConstruction 200) on a kdb_index_build graph, with 5 %
and 20 % of the nodes deleted at random, the entry point among them.

Per deleted fraction, in ONE process, every variant from the same built graph and the same deletes (the builder is
deterministic: the graph is built again for each variant):
  (a) the tombstoned graph                       -- the behaviour before there was a vacuum: the baseline
  (r) kdb_index_refine over the census' nodes    -- the repair alone (same R), the yardstick of the vacuum's wall time
  (b) kdb_index_vacuum, the reference's entry rule (lowest live id, its level)
  (c) kdb_index_vacuum with KDB_VACUUM_ELECT_TOP_LEVEL
  (d) a fresh kdb_index_build over the survivors only -- the ceiling
recall@10 against the exact scan over the survivors and QPS at the headline's ef / batch: 3 warm-up launches, then 10 timed
ones, the median of their HIP-event times (kdb_get_launch_stats); n_dist per query of the last launch (kdb_get_counters).
Wall times (host clock around calls that end in a device synchronise): dead_link_scan (kernel + 125 KB read-back), refine over
R, vacuum (scan + repair + cleanup + election).  The per-kernel split -- vacuum_scan_kernel beside (adjacency bytes) /
(kdb_probe_stream's bandwidth of this run), vacuum_clear_kernel, refine's three -- comes from one more 5 % vacuum in a child
process under `rocprofv3 --kernel-trace`.

usage: python scripts/vacuum_probe.py [--rows N] [--out profiles/vacuum_probe.json]"""
import argparse
import glob
import json
import os
import shutil
import sqlite3
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import kektordb_amd as K  # noqa: E402
from bench import gen_corpus, recall_at_k, outs  # noqa: E402

KERNELS = ("vacuum_scan_kernel", "vacuum_clear_kernel", "refine_search_kernel", "refine_select_kernel", "refine_commit_kernel")


def log(*a):
    print("[vacuum_probe]", *a, file=sys.stderr, flush=True)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


def exact(idx, Q, k, dev, allow=None):
    o = outs(Q.shape[0], k, dev)
    idx.flat_scan_batch_dev(Q, k, *o, d_allow=allow)
    idx.sync()
    return o[0].cpu().numpy().view(np.uint32)


def measure(idx, QB, Qr, gt, k, ef, dev, id_map=None):
    """recall@k on the recall queries Qr; kernel time / QPS / n_dist per query of the headline batch QB"""
    o = outs(Qr.shape[0], k, dev)
    idx.search_batch_dev(Qr, k, ef, *o)
    idx.sync()
    ids = o[0].cpu().numpy().view(np.uint32)
    cnt = o[2].cpu().numpy()
    if id_map is not None:
        ids = id_map[ids]
    for b in range(ids.shape[0]):                               # (unused slots must not count as hits)
        ids[b, int(cnt[b]):] = 0xffffffff
    rec = round(recall_at_k(ids, gt, k), 4)
    ob = outs(QB.shape[0], k, dev)
    for _ in range(3):
        idx.search_batch_dev(QB, k, ef, *ob)
    idx.sync()
    reps = 10
    for _ in range(reps):
        idx.search_batch_dev(QB, k, ef, *ob)
    idx.sync()
    ms = [s["kernel_ms"] for s in idx.launch_stats(reps)]
    c = idx.counters()
    med = statistics.median(ms)
    return {"recall_at_10": rec, "kernel_ms_median": round(med, 3), "kernel_ms_min_max": [round(min(ms), 3), round(max(ms), 3)],
            "qps": round(QB.shape[0] / (med * 1e-3)), "n_dist_per_query": round(c["n_dist"] / QB.shape[0], 1),
            "n_hops_per_query": round(c["n_hops"] / QB.shape[0], 1), "n_dropped": c["n_dropped"]}


def kernel_split(a):
    """{kernel: launches, total ms} of one 5 % vacuum, from a child under rocprofv3 --kernel-trace (None when it is not there)"""
    if shutil.which("rocprofv3") is None:
        return None
    out = f"/tmp/kdb_vacuum_probe_{os.getpid()}"
    shutil.rmtree(out, ignore_errors=True)
    cmd = ["rocprofv3", "--kernel-trace", "-d", out, "-o", "p", "--", sys.executable, os.path.abspath(__file__), "--split-child",
           "--rows", str(a.rows), "--dim", str(a.dim), "--efc", str(a.efc)]
    try:
        p = subprocess.run(cmd, cwd="/tmp", env=dict(os.environ, TMPDIR="/tmp"), capture_output=True, text=True, timeout=420)
        dbs = glob.glob(os.path.join(out, "**", "*.db"), recursive=True)
        if p.returncode != 0 or not dbs:
            log(f"kernel trace failed (rc {p.returncode}): {p.stderr[-300:]}")
            return None
        rows = sqlite3.connect(dbs[0]).cursor().execute("select name, count(*), sum(duration) from kernels group by name").fetchall()
        split = {}
        for name, calls, ns in rows:
            for key in KERNELS:
                if key in name:
                    e = split.setdefault(key, {"launches": 0, "ms": 0.0})
                    e["launches"] += int(calls)
                    e["ms"] = round(e["ms"] + ns / 1e6, 3)
        return split
    except Exception as e:  # the timings above are the probe's point: never lose them
        log(f"kernel trace failed: {e!r}")
        return None
    finally:
        shutil.rmtree(out, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--efc", type=int, default=200)
    ap.add_argument("--ef", type=int, default=60)
    ap.add_argument("--batch", type=int, default=32768)
    ap.add_argument("--queries", type=int, default=2048)
    ap.add_argument("--fractions", default="0.05,0.20")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vacuum_probe.json"))
    ap.add_argument("--no-split", action="store_true")
    ap.add_argument("--split-child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    n, dim, k = a.rows, a.dim, 10
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    centers = torch.randn((4096, dim), device=dev, generator=g)
    X = gen_corpus(n, dim, "clustered", 1000, dev, centers)
    idx = K.HipIndex(dim, K.COSINE, K.F32, 16, a.efc, capacity=n)
    idx.upload_rows(X, 1)

    def start(frac):
        """the built graph with its deletes -> the deleted ids (always the same: seeded, the entry point first)"""
        idx.upload_rows(X, 1)                                   # (a vacuum zeroed the rows of the deleted nodes)
        idx.build(n, batch=16384, ef_construction=a.efc, seed=1)
        rng = np.random.default_rng(77)
        dead = rng.choice(np.arange(1, n + 1), int(n * frac), replace=False).astype(np.uint32)
        entry = idx.graph_info()[1]
        if entry not in dead:
            dead[0] = entry
        idx.Delete(dead)
        return dead

    if a.split_child:
        start(0.05)
        idx.vacuum(ef_construction=a.efc)
        idx.sync()
        return
    Qr = gen_corpus(a.queries, dim, "clustered", 4242, dev, centers)
    QB = gen_corpus(a.batch, dim, "clustered", 4243, dev, centers)
    res = {"rows": n, "dim": dim, "metric": "cosine", "corpus": "clustered-4096 + 0.3*N(0,1), L2-normalised", "m": 16, "ef_construction": a.efc,
           "ef_search": a.ef, "batch": a.batch, "recall_queries": a.queries,
           "timing": "kernel_ms: HIP events of kdb_get_launch_stats, median of 10 launches after 3 warm-ups; *_s: host clock around a call that ends in a device synchronise"}
    res["stream_GBps"] = round(idx.probe_stream(), 1)
    runs = {}
    for frac in [float(f) for f in a.fractions.split(",")]:
        r = {}
        dead = start(frac)
        allow = np.full((n >> 6) + 1, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
        np.bitwise_and.at(allow, (dead >> 6).astype(np.int64), ~(np.uint64(1) << (dead & 63).astype(np.uint64)))
        gt = exact(idx, Qr, k, dev, allow=torch.from_numpy(allow.view(np.int64)).to(dev))
        levels = idx.download_graph()[3]
        adj_bytes = (n + 1) * 32 * 4 + int(levels[1:].astype(np.int64).sum()) * 16 * 4
        r["a_tombstoned"] = measure(idx, QB, Qr, gt, k, a.ef, dev)
        log(frac, "a", r["a_tombstoned"])
        t_scan = []
        for _ in range(5):                                      # the first call grows the scratch
            t, (ids, links, nd) = timed(lambda: idx.dead_link_scan())
            t_scan.append(t)
        r["census"] = {"dead_nodes": nd, "nodes_with_dead_links": int(ids.size), "dead_links": links, "live_nodes": n - nd,
                       "dead_link_scan_s": {"median": round(statistics.median(t_scan), 5), "runs": [round(t, 5) for t in t_scan]},
                       "adjacency_bytes": adj_bytes, "adjacency_bytes_over_stream_bandwidth_ms": round(adj_bytes / (res["stream_GBps"] * 1e9) * 1e3, 4)}
        t, st = timed(lambda: idx.refine(ids, ef_construction=a.efc))
        r["r_refine_same_R"] = {"seconds": round(t, 3), **st, **measure(idx, QB, Qr, gt, k, a.ef, dev)}
        log(frac, "r", r["r_refine_same_R"])
        for key, top in (("b_vacuum_reference_rule", False), ("c_vacuum_elect_top_level", True)):
            start(frac)
            t, st = timed(lambda: idx.vacuum(ef_construction=a.efc, elect_top_level=top))
            assert st["dead_links_found"] == st["dead_links_dropped"] == links and st["nodes_repaired"] == ids.size, st
            t2, st2 = timed(lambda: idx.vacuum(ef_construction=a.efc, elect_top_level=top))
            assert st2["nodes_repaired"] == 0, st2
            r[key] = {"seconds": round(t, 3), "second_call_seconds": round(t2, 4), **st, **measure(idx, QB, Qr, gt, k, a.ef, dev)}
            log(frac, key, r[key])
        r["vacuum_minus_refine_s"] = round(r["b_vacuum_reference_rule"]["seconds"] - r["r_refine_same_R"]["seconds"], 4)
        # (d) the survivors alone, built from scratch
        live = np.setdiff1d(np.arange(1, n + 1, dtype=np.uint32), dead)
        fresh = K.HipIndex(dim, K.COSINE, K.F32, 16, a.efc, capacity=live.size)
        fresh.upload_rows(X[torch.from_numpy((live - 1).astype(np.int64)).to(dev)].contiguous(), 1)
        t, _ = timed(lambda: fresh.build(int(live.size), batch=16384, ef_construction=a.efc, seed=1))
        id_map = np.concatenate([np.zeros(1, np.uint32), live])
        r["d_fresh_build_of_survivors"] = {"build_seconds": round(t, 3), **measure(fresh, QB, Qr, gt, k, a.ef, dev, id_map=id_map)}
        log(frac, "d", r["d_fresh_build_of_survivors"])
        fresh.Close()
        del fresh
        torch.cuda.empty_cache()
        runs[f"{frac:g}"] = r
    res["deleted_fraction"] = runs
    idx.Close()
    del X
    torch.cuda.empty_cache()
    res["kernel_split_ms_one_vacuum_5pct"] = None if a.no_split else kernel_split(a)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
