"""kdb_index_add on the headline corpus (1M x 768 cosine, clustered, m 16, efConstruction 200), next to the CPU restatement.

The graph is the GPU builder's over the first rows - 4000 rows; the last 4000 rows are held out (uploaded, not in the graph).
  * latency     2000 held-out rows, one kdb_index_add call each (n = 1): median and p99 wall time of the C call;
  * throughput  the other 2000 in ONE call: nodes per second;
  * CPU         the oracle's add (orc_index_add: the reference's Add restated) of the first 2000 held-out rows into the same
                graph as downloaded before the GPU inserts, same forced levels, single thread, AVX2 arithmetic (ARITH_RUST, as
                bench.py times the CPU search): median and p99 per add, adds per second.
The kernel-time split (add_link_kernel = walk + forward select, add_reverse_kernel) comes from a child process under
`rocprofv3 --kernel-trace` that repeats the inserts.  Every step that uses the GPU is a child process under its own time limit;
a step that fails ends the probe.

usage: python scripts/add_probe.py [--rows N] [--out profiles/add_probe.json]"""
import argparse
import ctypes as C
import glob
import json
import os
import shutil
import sqlite3
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HELD = 4000


def log(*a):
    print("[add_probe]", *a, file=sys.stderr, flush=True)


def pct(x, p):
    return round(float(np.percentile(np.asarray(x), p)) * 1e3, 4)  # ms


def setup(a):
    """corpus on the device, the builder's graph over the first rows - HELD rows, levels of the held-out rows"""
    import torch
    import kektordb_amd as K
    from bench import gen_corpus
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    centers = torch.randn((4096, a.dim), device=dev, generator=g)
    X = gen_corpus(a.rows, a.dim, "clustered", 1000, dev, centers)
    idx = K.HipIndex(a.dim, K.COSINE, K.F32, 16, a.efc, capacity=a.rows)
    idx.upload_rows(X, 1)
    base = a.rows - HELD
    t0 = time.perf_counter()
    idx.build(base, batch=16384, ef_construction=a.efc, seed=1)
    idx.sync()
    log(f"built {base} rows in {time.perf_counter() - t0:.1f} s")
    rng = np.random.default_rng(77)
    levels = np.minimum(np.floor(-np.log(1.0 - rng.random(HELD)) / np.log(16)), 255).astype(np.uint8)
    return idx, base, levels


def step_measure(a):
    from oracle import oracle as O
    idx, base, levels = setup(a)
    res = {"rows": a.rows, "graph_rows": base, "dim": a.dim, "metric": "cosine", "corpus": "clustered-4096 + 0.3*N(0,1), L2-normalised", "m": 16,
           "ef_construction": a.efc}
    half = HELD // 2
    # ---- the CPU side first: it needs the graph as it is before the inserts
    count, entry, max_level, glv, offs, nbrs = idx.download_graph()
    rows = np.zeros((a.rows + 1, a.dim), dtype=np.float32)
    rows[1:] = idx.download_rows(1, a.rows)
    L = O.lib()
    offs = [np.ascontiguousarray(o, dtype=np.uint64) for o in offs]
    nbrs = [np.ascontiguousarray(x if x.size else np.zeros(1, np.uint32), dtype=np.uint32) for x in nbrs]
    nl = max_level + 1
    op = (C.c_void_p * max(nl, 1))(*[o.ctypes.data for o in offs])
    npp = (C.c_void_p * max(nl, 1))(*[x.ctypes.data for x in nbrs])
    dbits = np.zeros((count >> 6) + 1, dtype=np.uint64)
    # (the rows are borrowed: the buffer already holds the held-out rows behind the graph's, where Add stores them again)
    h = L.orc_index_from_graph(a.dim, O.COSINE, O.F32, 16, a.efc, rows.ctypes.data_as(C.c_void_p), None, count, glv.ctypes.data_as(C.c_void_p),
                               max_level, entry, op, npp, dbits.ctypes.data_as(C.c_void_p), C.c_float(0.0))
    assert h
    L.orc_index_set_arith(h, O.ARITH_RUST)
    held = rows[base + 1:base + 1 + half].copy()
    t_cpu = []
    for i in range(a.cpu_adds):
        t0 = time.perf_counter()
        L.orc_index_add(h, held[i].ctypes.data_as(C.c_void_p), int(levels[i]))
        t_cpu.append(time.perf_counter() - t0)
    L.orc_index_free(h)
    res["cpu_add"] = {"adds": a.cpu_adds, "threads": 1, "arith": "AVX2 (ARITH_RUST)", "median_ms": pct(t_cpu, 50), "p99_ms": pct(t_cpu, 99),
                      "adds_per_s": round(len(t_cpu) / sum(t_cpu), 1)}
    log("cpu", res["cpu_add"])
    del rows, held
    # ---- latency: one call per node
    for i in range(8):  # (warm-up on the first nodes: code objects, LDS attributes, the visited set)
        idx.add(base + 1 + i, levels[i:i + 1], a.efc)
    # (the C call itself is timed -- arguments prepared outside the clock -- not HipIndex.add's numpy / dict work around it)
    from kektordb_amd import _lib
    par, st1, t_gpu = _lib.AddParams(a.efc, 0), _lib.AddStats(), []
    for i in range(8, half):
        lvp = C.c_void_p(levels.ctypes.data + i)
        t0 = time.perf_counter()
        rc = idx.L.kdb_index_add(idx.h, base + 1 + i, 1, lvp, C.byref(par), C.byref(st1))
        t_gpu.append(time.perf_counter() - t0)
        assert rc == 0, rc
    res["gpu_add_n1"] = {"adds": len(t_gpu), "median_ms": pct(t_gpu, 50), "p99_ms": pct(t_gpu, 99), "adds_per_s": round(len(t_gpu) / sum(t_gpu), 1)}
    log("gpu n=1", res["gpu_add_n1"])
    # ---- throughput: one call
    t0 = time.perf_counter()
    stats = idx.add(base + 1 + half, levels[half:], a.efc)
    dt = time.perf_counter() - t0
    res["gpu_add_one_call"] = {"nodes": HELD - half, "seconds": round(dt, 4), "nodes_per_s": round((HELD - half) / dt, 1), "stats": stats}
    log("gpu one call", res["gpu_add_one_call"])
    res["gpu_over_cpu_latency"] = round(res["cpu_add"]["median_ms"] / res["gpu_add_n1"]["median_ms"], 3)
    print(json.dumps(res))


def step_split(a):
    """under rocprofv3 --kernel-trace: the same inserts once more"""
    idx, base, levels = setup(a)
    half = HELD // 2
    for i in range(half):
        idx.add(base + 1 + i, levels[i:i + 1], a.efc)
    idx.add(base + 1 + half, levels[half:], a.efc)
    idx.sync()


def child(a, step, limit, wrap=()):
    cmd = [*wrap, sys.executable, os.path.abspath(__file__), "--step", step, "--rows", str(a.rows), "--dim", str(a.dim), "--efc", str(a.efc),
           "--cpu-adds", str(a.cpu_adds)]
    log("step", step, "limit", limit, "s")
    return subprocess.run(cmd, capture_output=True, text=True, timeout=limit, cwd="/tmp" if wrap else ROOT, env=dict(os.environ, TMPDIR="/tmp"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--efc", type=int, default=200)
    ap.add_argument("--cpu-adds", type=int, default=HELD // 2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "add_probe.json"))
    ap.add_argument("--no-split", action="store_true")
    ap.add_argument("--step", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.step == "measure":
        return step_measure(a)
    if a.step == "split":
        return step_split(a)
    p = child(a, "measure", 900)
    sys.stderr.write(p.stderr[-4000:])
    if p.returncode != 0:
        log(f"the measurement failed (rc {p.returncode}): nothing more is started")
        sys.exit(1)
    res = json.loads(p.stdout.strip().splitlines()[-1])
    res["kernel_split_ms"] = None
    if not a.no_split and shutil.which("rocprofv3") is not None:
        out = f"/tmp/kdb_add_probe_{os.getpid()}"
        shutil.rmtree(out, ignore_errors=True)
        try:
            p = child(a, "split", 600, wrap=("rocprofv3", "--kernel-trace", "-d", out, "-o", "p", "--"))
            dbs = glob.glob(os.path.join(out, "**", "*.db"), recursive=True)
            if p.returncode == 0 and dbs:
                split = {}
                for name, calls, ns in sqlite3.connect(dbs[0]).cursor().execute("select name, count(*), sum(duration) from kernels group by name").fetchall():
                    for key in ("add_link_kernel", "add_reverse_kernel"):
                        if key in name:
                            e = split.setdefault(key, {"launches": 0, "ms": 0.0})
                            e["launches"] += int(calls)
                            e["ms"] = round(e["ms"] + ns / 1e6, 2)
                res["kernel_split_ms"] = split
            else:
                log(f"kernel trace failed (rc {p.returncode}): {p.stderr[-300:]}")
        except Exception as e:  # the timings above are the probe's point: never lose them
            log(f"kernel trace failed: {e!r}")
        finally:
            shutil.rmtree(out, ignore_errors=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
