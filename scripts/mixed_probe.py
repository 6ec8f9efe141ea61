"""Mixed search requests on the headline corpus (1M x 768 cosine, clustered, m 16, efConstruction 200): what per-query k and ef cost
the launches that do not use them, and what they buy the ones that do.  ONE process, callers as threads, the legs of every
comparison ALTERNATE, medians of --reps (31) with the spread as (min, max).

  1. homogeneous   32768 resident queries, k 10, ef 60 through kdb_search_batch_dev (host clock around call + sync), and 64 one-key
                   callers (one query per kdb_search_batch call): this build against the PARENT's (--parent-lib, a build of the parent
                   commit loaded beside this one: its own handle, the same rows and graph).  The parent's leg runs twice per round:
                   the difference between its two medians is the noise this build's median has to lie within.
  2. mixed callers 64 and 256 threads, one query per call, five keys inside one beam class (ef <= 64) and five keys over three
                   classes: combining across keys on (the default) against a handle created under KDB_COMBINE_MIXED=0, and the parent.
  3. mixed page    32768 queries with the five-key mixture in ONE kdb_search_batch_mixed against the same queries sorted by key into
                   five kdb_search_batch calls (host pointers, sum of the five).

The measurement runs in a child process under its own time limit; a step that fails ends the probe.

usage: python scripts/mixed_probe.py --parent-lib /path/to/parent/libkektor_hip.so [--rows N] [--out profiles/mixed_probe.json]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KEYS_ONE_CLASS = [(10, 48), (5, 20), (10, 64), (3, 30), (20, 40)]        # effective ef <= 64: one register slot
KEYS_THREE_CLASSES = [(10, 48), (5, 20), (20, 64), (10, 100), (3, 130)]   # 64 | 128 | 256


def log(*a):
    print("[mixed_probe]", *a, file=sys.stderr, flush=True)


def ms(x):
    x = np.asarray(x) * 1e3
    return {"median_ms": round(float(np.median(x)), 4), "min_ms": round(float(x.min()), 4), "max_ms": round(float(x.max()), 4)}


def med(x):
    x = np.asarray(x, dtype=np.float64)
    return {"median": round(float(np.median(x)), 1), "min": round(float(x.min()), 1), "max": round(float(x.max()), 1)}


def index_on_library(K, path, dim, efc, cap):
    """a HipIndex whose calls go to ANOTHER build of the library (the parent's: it lacks the entry points this build adds, so only
    the ones the probe uses are declared)"""
    from kektordb_amd import _lib
    L = C.CDLL(path)
    vp, u32 = C.c_void_p, C.c_uint32
    L.kdb_last_error.restype = C.c_char_p
    L.kdb_index_create.argtypes = [C.POINTER(_lib.IndexDesc), C.POINTER(vp)]
    L.kdb_index_destroy.argtypes = [vp]
    L.kdb_index_destroy.restype = None
    L.kdb_index_upload_rows_dev.argtypes = [vp, u32, u32, vp]
    L.kdb_index_upload_graph.argtypes = [vp, C.POINTER(_lib.GraphView)]
    L.kdb_search_batch.argtypes = [vp, vp, u32, u32, u32, vp, u32, vp, vp, vp]
    L.kdb_search_batch_dev.argtypes = [vp, vp, u32, u32, u32, vp, u32, vp, vp, vp, vp]
    L.kdb_index_caller_stats.argtypes = [vp, vp]
    L.kdb_index_sync.argtypes = [vp]
    idx = K.HipIndex.__new__(K.HipIndex)
    idx.L, idx.dim, idx.metric, idx.precision, idx.m, idx.ef_construction, idx.capacity = L, dim, K.COSINE, K.F32, 16, efc, cap
    idx.device_id, idx.needs_refine, idx._closed = 0, False, False
    desc = _lib.IndexDesc(dim, K.COSINE, K.F32, 16, efc, cap, 0, 0)
    h = C.c_void_p()
    rc = L.kdb_index_create(C.byref(desc), C.byref(h))
    assert rc == 0, (rc, L.kdb_last_error())
    idx.h = h
    return idx


def run_callers(idx, Q, keys, n_threads, seconds):
    """n_threads threads, one query per kdb_search_batch call, keys drawn per call; -> (QPS, latencies in seconds)"""
    L, h, dim = idx.L, idx.h, Q.shape[1]
    lat = [[] for _ in range(n_threads)]
    start = threading.Barrier(n_threads + 1)
    stop = [0.0]
    errs = []

    def caller(t):
        rng = np.random.default_rng(100 + t)
        kmax = max(k for k, _ in keys)
        ids, dist, cnt = np.zeros(kmax, np.uint32), np.zeros(kmax, np.float32), np.zeros(1, np.uint32)
        pi, pd, pc = (x.ctypes.data_as(C.c_void_p) for x in (ids, dist, cnt))
        order = rng.integers(0, len(keys), 4096)
        rows = rng.integers(0, Q.shape[0], 4096)
        base = Q.ctypes.data
        mine = lat[t]
        start.wait()
        i = 0
        while True:
            t0 = time.perf_counter()
            if t0 >= stop[0]:
                break
            k, ef = keys[order[i & 4095]]
            rc = L.kdb_search_batch(h, C.c_void_p(base + int(rows[i & 4095]) * dim * 4), 1, k, ef, None, 0, pi, pd, pc)
            if rc:
                errs.append(rc)
                break
            mine.append(time.perf_counter() - t0)
            i += 1

    ts = [threading.Thread(target=caller, args=(t,)) for t in range(n_threads)]
    for t in ts:
        t.start()
    stop[0] = time.perf_counter() + seconds + 0.05
    start.wait()
    t0 = time.perf_counter()
    for t in ts:
        t.join()
    el = time.perf_counter() - t0
    assert not errs, errs[:3]
    all_lat = np.concatenate([np.asarray(x) for x in lat if x]) if any(lat) else np.zeros(1)
    return len(all_lat) / el, all_lat


def caller_leg(handles, Q, keys, n_threads, reps, seconds):
    """handles: name -> index; the named legs alternate inside every round"""
    acc = {name: {"qps": [], "p50": [], "p99": []} for name in handles}
    for _ in range(reps):
        for name, idx in handles.items():
            qps, lat = run_callers(idx, Q, keys, n_threads, seconds)
            acc[name]["qps"].append(qps)
            acc[name]["p50"].append(float(np.percentile(lat, 50)) * 1e6)
            acc[name]["p99"].append(float(np.percentile(lat, 99)) * 1e6)
    return {name: {"qps": med(v["qps"]), "p50_us": med(v["p50"]), "p99_us": med(v["p99"])} for name, v in acc.items()}


def step_measure(a):
    import torch
    import kektordb_amd as K
    from bench import gen_corpus
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    centers = torch.randn((4096, a.dim), device=dev, generator=g)
    X = gen_corpus(a.rows, a.dim, "clustered", 1000, dev, centers)
    Qd = gen_corpus(a.queries, a.dim, "clustered", 2000, dev, centers)
    builder = K.HipIndex(a.dim, K.COSINE, K.F32, 16, a.efc, capacity=a.rows)
    builder.upload_rows(X, 1)
    t0 = time.perf_counter()
    builder.build(a.rows, batch=16384, ef_construction=a.efc, seed=1)
    builder.sync()
    log(f"built {a.rows} rows in {time.perf_counter() - t0:.1f} s")
    graph = builder.download_graph()
    builder.close()
    # every handle that is measured gets rows and graph the same way (uploaded), whichever build it belongs to
    child = K.HipIndex(a.dim, K.COSINE, K.F32, 16, a.efc, capacity=a.rows)
    os.environ["KDB_COMBINE_MIXED"] = "0"
    off = K.HipIndex(a.dim, K.COSINE, K.F32, 16, a.efc, capacity=a.rows)
    del os.environ["KDB_COMBINE_MIXED"]
    parent = index_on_library(K, a.parent_lib, a.dim, a.efc, a.rows)
    for idx in (child, off, parent):
        idx.upload_rows(X, 1)
        idx.upload_graph(*graph)
    del X, graph
    B, k, ef = a.queries, a.k, a.ef
    Q = Qd.cpu().numpy()
    res = {"rows": a.rows, "dim": a.dim, "metric": "cosine", "corpus": "clustered-4096 + 0.3*N(0,1), L2-normalised", "m": 16, "ef_construction": a.efc,
           "queries": B, "k": k, "ef": ef, "reps": a.reps, "caller_reps": a.caller_reps, "caller_seconds": a.caller_seconds,
           "keys_one_class": KEYS_ONE_CLASS, "keys_three_classes": KEYS_THREE_CLASSES}

    # ---- 1. the homogeneous path -------------------------------------------------------------------------------------------------
    out = {n: (torch.zeros((B, k), dtype=torch.int32, device=dev), torch.zeros((B, k), dtype=torch.float32, device=dev),
               torch.zeros(B, dtype=torch.int32, device=dev)) for n in ("child", "parent")}

    def resident(idx, o):
        t0 = time.perf_counter()
        idx.search_batch_dev(Qd, k, ef, *o)
        idx.sync()
        return time.perf_counter() - t0

    for _ in range(max(a.warmup, 1)):
        resident(child, out["child"])
        resident(parent, out["parent"])
    same = all(torch.equal(x, y) for x, y in zip(out["child"], out["parent"]))
    log(f"homogeneous answers of the two builds equal: {same}")
    assert same
    t = {"parent_a": [], "child": [], "parent_b": []}
    for _ in range(a.reps):
        t["parent_a"].append(resident(parent, out["parent"]))
        t["child"].append(resident(child, out["child"]))
        t["parent_b"].append(resident(parent, out["parent"]))
    res["homogeneous_resident"] = {n: ms(v) for n, v in t.items()}
    m = {n: float(np.median(v)) * 1e3 for n, v in t.items()}
    res["homogeneous_resident"]["parent_leg_to_leg_ms"] = round(abs(m["parent_a"] - m["parent_b"]), 4)
    res["homogeneous_resident"]["child_minus_parent_mean_ms"] = round(m["child"] - (m["parent_a"] + m["parent_b"]) / 2, 4)
    log("homogeneous resident:", json.dumps(res["homogeneous_resident"]))
    one_key = [(k, ef)]
    run_callers(child, Q, one_key, 64, 0.2)
    run_callers(parent, Q, one_key, 64, 0.2)
    res["homogeneous_64_callers"] = caller_leg({"parent_a": parent, "child": child, "parent_b": parent}, Q, one_key, 64, a.caller_reps, a.caller_seconds)
    log("homogeneous 64 callers:", json.dumps(res["homogeneous_64_callers"]))

    # ---- 2. mixed callers --------------------------------------------------------------------------------------------------------
    res["mixed_callers"] = {}
    for set_name, keys in (("one_class", KEYS_ONE_CLASS), ("three_classes", KEYS_THREE_CLASSES)):
        for n_threads in (64, 256):
            m0 = child.mixed_stats()
            leg = caller_leg({"on": child, "off": off}, Q, keys, n_threads, a.caller_reps, a.caller_seconds)
            leg["parent_once"] = caller_leg({"parent": parent}, Q, keys, n_threads, 1, a.caller_seconds)["parent"]
            leg["mixed_stats_on"] = [x - y for x, y in zip(child.mixed_stats(), m0)]
            res["mixed_callers"][f"{set_name}_{n_threads}"] = leg
            log(f"mixed callers {set_name} x {n_threads}:", json.dumps(leg))

    # ---- 3. a mixed page ---------------------------------------------------------------------------------------------------------
    keys = KEYS_THREE_CLASSES
    which = np.random.default_rng(3).integers(0, len(keys), B)
    ks = np.array([keys[i][0] for i in which], np.uint32)
    efs = np.array([keys[i][1] for i in which], np.uint32)
    order = np.argsort(which, kind="stable")
    Qs = np.ascontiguousarray(Q[order])
    bounds = np.searchsorted(which[order], np.arange(len(keys) + 1))

    def page_mixed():
        t0 = time.perf_counter()
        r = child.search_batch_mixed(Q, ks, efs)
        return time.perf_counter() - t0, r

    def page_sorted():
        t0 = time.perf_counter()
        r = [child.search_batch(Qs[bounds[i]:bounds[i + 1]], keys[i][0], keys[i][1]) for i in range(len(keys))]
        return time.perf_counter() - t0, r

    _, rm = page_mixed()
    _, rs = page_sorted()
    for i in range(len(keys)):   # the same answers either way
        sel = order[bounds[i]:bounds[i + 1]]
        kk = keys[i][0]
        assert np.array_equal(rm[0][sel][:, :kk], rs[i][0]) and np.array_equal(rm[2][sel], rs[i][2]), i
    tm, tsrt = [], []
    for _ in range(a.reps):
        tm.append(page_mixed()[0])
        tsrt.append(page_sorted()[0])
    res["mixed_page"] = {"one_mixed_call": ms(tm), "five_sorted_calls": ms(tsrt), "answers_equal": True,
                         "mixed_over_sorted": round(float(np.median(tm)) / float(np.median(tsrt)), 3)}
    log("mixed page:", json.dumps(res["mixed_page"]))
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True, help="libkektor_hip.so built from the parent commit")
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--efc", type=int, default=200)
    ap.add_argument("--queries", type=int, default=32768)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--ef", type=int, default=60)
    ap.add_argument("--reps", type=int, default=31)
    ap.add_argument("--caller-reps", type=int, default=31)
    ap.add_argument("--caller-seconds", type=float, default=0.25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--limit", type=int, default=900, help="seconds the measurement may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mixed_probe.json"))
    ap.add_argument("--step", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.step == "measure":
        return step_measure(a)
    cmd = [sys.executable, os.path.abspath(__file__), "--step", "measure", "--parent-lib", os.path.abspath(a.parent_lib)]
    for key in ("rows", "dim", "efc", "queries", "k", "ef", "reps", "caller_reps", "caller_seconds", "warmup"):
        cmd += ["--" + key.replace("_", "-"), str(getattr(a, key))]
    log(f"step measure, limit {a.limit} s")
    p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=a.limit, cwd=ROOT)
    if p.returncode != 0:
        log(f"the measurement failed (rc {p.returncode}): nothing more is started")
        sys.exit(1)
    res = json.loads(p.stdout.strip().splitlines()[-1])
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
