"""kdb_index_refine next to kdb_index_build on the headline corpus (1M x 768 cosine, clustered, efConstruction 200).

Times, in ONE process, as medians of 3 with hipDeviceSynchronize around each call:
  * kdb_index_build over the rows (the yardstick: refine does one efC walk and one select per (node, level) and no
    reverse-link phase, so it has no reason to cost more);
  * kdb_index_refine over all nodes of that graph (every run starts from a freshly built graph: a refined graph walks differently).
The per-kernel split comes from one more build + refine in a child process under `rocprofv3 --kernel-trace`.
Recall@10 at ef 60 against the exact scan: before / after refining a graph linked by kdb_index_add_batch, and, after deleting
20 % of its nodes, before / after refining again (ground truth over the live rows).

usage: python scripts/refine_probe.py [--rows N] [--out profiles/refine_probe.json]"""
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


def log(*a):
    print("[refine_probe]", *a, file=sys.stderr, flush=True)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


def search_recall(idx, Q, gt, k, ef, dev):
    o = outs(Q.shape[0], k, dev)
    idx.search_batch_dev(Q, k, ef, *o)
    idx.sync()
    return round(recall_at_k(o[0].cpu().numpy().view(np.uint32), gt, k), 4)


def exact(idx, Q, k, dev, allow=None):
    o = outs(Q.shape[0], k, dev)
    idx.flat_scan_batch_dev(Q, k, *o, d_allow=allow)
    idx.sync()
    return o[0].cpu().numpy().view(np.uint32)


def kernel_split(a):
    """{kernel: total ms} of one build + one refine, from a child under rocprofv3 --kernel-trace (None when it is not there)"""
    if shutil.which("rocprofv3") is None:
        return None
    out = f"/tmp/kdb_refine_probe_{os.getpid()}"
    shutil.rmtree(out, ignore_errors=True)
    cmd = ["rocprofv3", "--kernel-trace", "-d", out, "-o", "p", "--", sys.executable, os.path.abspath(__file__), "--split-child",
           "--rows", str(a.rows), "--dim", str(a.dim), "--efc", str(a.efc)]
    try:
        p = subprocess.run(cmd, cwd="/tmp", env=dict(os.environ, TMPDIR="/tmp"), capture_output=True, text=True, timeout=420)
        dbs = glob.glob(os.path.join(out, "**", "*.db"), recursive=True)
        if p.returncode != 0 or not dbs:
            print(f"[refine_probe] kernel trace failed (rc {p.returncode}): {p.stderr[-300:]}", file=sys.stderr)
            return None
        rows = sqlite3.connect(dbs[0]).cursor().execute("select name, count(*), sum(duration) from kernels group by name").fetchall()
        split = {}
        for name, calls, ns in rows:
            for key in ("build_search_kernel", "build_select_kernel", "build_reverse_kernel", "refine_search_kernel", "refine_select_kernel",
                        "refine_commit_kernel"):
                if key in name:
                    e = split.setdefault(key, {"launches": 0, "ms": 0.0})
                    e["launches"] += int(calls)
                    e["ms"] = round(e["ms"] + ns / 1e6, 2)
        return split
    except Exception as e:  # the timings above are the probe's point: never lose them
        print(f"[refine_probe] kernel trace failed: {e!r}", file=sys.stderr)
        return None
    finally:
        shutil.rmtree(out, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--efc", type=int, default=200)
    ap.add_argument("--ef", type=int, default=60)
    ap.add_argument("--queries", type=int, default=2048)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refine_probe.json"))
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
    if a.split_child:
        idx.build(n, batch=16384, ef_construction=a.efc, seed=1)
        idx.refine(ef_construction=a.efc)
        idx.sync()
        return
    Q = gen_corpus(a.queries, dim, "clustered", 4242, dev, centers)
    res = {"rows": n, "dim": dim, "metric": "cosine", "corpus": "clustered-4096 + 0.3*N(0,1), L2-normalised", "m": 16, "ef_construction": a.efc,
           "ef_search": a.ef, "queries": a.queries}
    # ---- build and refine, same process, medians of 3
    t_build, t_refine, stats = [], [], None
    for _ in range(3):
        t, _ = timed(lambda: idx.build(n, batch=16384, ef_construction=a.efc, seed=1))
        t_build.append(t)
        t, stats = timed(lambda: idx.refine(ef_construction=a.efc))
        t_refine.append(t)
        log(f"build {t_build[-1]:.3f} s, refine {t_refine[-1]:.3f} s", stats)
    gt = exact(idx, Q, k, dev)
    res["build_s"] = {"median": round(statistics.median(t_build), 3), "runs": [round(t, 3) for t in t_build]}
    res["refine_s"] = {"median": round(statistics.median(t_refine), 3), "runs": [round(t, 3) for t in t_refine]}
    res["refine_over_build"] = round(statistics.median(t_refine) / statistics.median(t_build), 3)
    res["refine_stats"] = stats
    # the fast builder's graph: as built, refined once, refined twice (links are one-directional: what does a second pass do?)
    fb = {"refined": search_recall(idx, Q, gt, k, a.ef, dev)}
    idx.refine(ef_construction=a.efc)
    fb["refined_twice"] = search_recall(idx, Q, gt, k, a.ef, dev)
    idx.build(n, batch=16384, ef_construction=a.efc, seed=1)
    fb["as_built"] = search_recall(idx, Q, gt, k, a.ef, dev)
    res["recall_at_10_fast_builder_graph"] = fb
    log("fast builder graph", fb)
    # ---- recall on a graph linked by kdb_index_add_batch, before / after refine, then with 20 % deleted
    first = max(a.efc, 1000)
    idx.build(first, batch=512, ef_construction=a.efc, seed=1)
    rng = np.random.default_rng(77)
    levels = np.minimum(np.floor(-np.log(1.0 - rng.random(n)) / np.log(16)), 255).astype(np.uint8)
    t0 = time.perf_counter()
    for pos in range(first, n, 5000):
        idx.add_batch(pos + 1, levels[pos:pos + min(5000, n - pos)], a.efc)
    idx.sync()
    res["add_batch_graph_s"] = round(time.perf_counter() - t0, 2)
    rec = {"add_batch_graph": search_recall(idx, Q, gt, k, a.ef, dev)}
    log("add_batch graph", res["add_batch_graph_s"], "s", rec)
    t, st = timed(lambda: idx.refine(ef_construction=a.efc))
    rec["add_batch_graph_refined"] = search_recall(idx, Q, gt, k, a.ef, dev)
    res["refine_of_add_batch_graph"] = {"seconds": round(t, 3), **st}
    dead = rng.choice(np.arange(1, n + 1), n // 5, replace=False).astype(np.uint32)
    idx.Delete(dead)
    allow = np.full((n >> 6) + 1, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
    np.bitwise_and.at(allow, (dead >> 6).astype(np.int64), ~(np.uint64(1) << (dead & 63).astype(np.uint64)))
    gt_live = exact(idx, Q, k, dev, allow=torch.from_numpy(allow.view(np.int64)).to(dev))
    rec["after_deleting_20pct"] = search_recall(idx, Q, gt_live, k, a.ef, dev)
    t, st = timed(lambda: idx.refine(ef_construction=a.efc))
    rec["after_deleting_20pct_refined"] = search_recall(idx, Q, gt_live, k, a.ef, dev)
    res["refine_after_deletes"] = {"seconds": round(t, 3), **st}
    res["recall_at_10"] = rec
    log(rec)
    idx.Close()
    del X
    torch.cuda.empty_cache()
    res["kernel_split_ms_one_build_one_refine"] = None if a.no_split else kernel_split(a)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
