"""The belief-state request on the headline corpus (1M x 768 cosine, clustered, m 16, efConstruction 200): 4096 queries, k = 10 and
k = 50, ef 100 -- Engine.VBeliefState's search, VGet of the k results and CalculateConsensus (pkg/engine/epistemic.go:22-182).

  * belief              kdb_belief_batch: one call, the k rows of every query never leave the device;
  * search_consensus    kdb_search_batch, then kdb_consensus_batch on its ids and counts;
  * host                today's way: kdb_search_batch, kdb_index_decode_rows of the B x k result ids (k x dim x 4 bytes per query come
                        out), then consensus_host (include/kektor_hip.hpp) on one thread and on 16.

Host pointers everywhere, pageable numpy buffers, a host clock around calls that end in a stream synchronise.  The legs ALTERNATE in
one process, --reps times after --warmup rounds; medians, and the spread as (min, max).  The consensus kernel alone is timed with
events around kdb_consensus_batch_dev on device buffers.  Before anything is timed the two device ways must agree bit for bit and
the host way within the bounds of tests/test_gpu_consensus.py.  The measurement runs in a child process under its own time limit.

usage: python scripts/consensus_probe.py [--rows N] [--queries B] [--out profiles/consensus_probe.json]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def log(*a):
    print("[consensus_probe]", *a, file=sys.stderr, flush=True)


def ms(x):
    x = np.asarray(x) * 1e3
    return {"median_ms": round(float(np.median(x)), 4), "min_ms": round(float(x.min()), 4), "max_ms": round(float(x.max()), 4)}


def host_shim():
    d = tempfile.mkdtemp(prefix="consensus_probe_")
    so = os.path.join(d, "consensus_host_shim.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-pthread", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "scripts", "consensus_host_shim.cpp"), "-o", so], check=True)
    return C.CDLL(so)


def step_measure(a):
    import torch
    import kektordb_amd as K
    from kektordb_amd.index import CONSENSUS_DTYPE
    from bench import gen_corpus
    shim = host_shim()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    centers = torch.randn((4096, a.dim), device=dev, generator=g)
    X = gen_corpus(a.rows, a.dim, "clustered", 1000, dev, centers)
    idx = K.HipIndex(a.dim, K.COSINE, K.F32, 16, a.efc, capacity=a.rows)
    idx.upload_rows(X, 1)
    B, ef, dim = a.queries, a.ef, a.dim
    rng = np.random.default_rng(3)
    pick = torch.from_numpy(rng.choice(a.rows, B, replace=False)).to(dev)
    Q = (X[pick] + 0.05 * torch.randn((B, dim), device=dev, generator=g)).cpu().numpy().astype(np.float32)
    del X
    t0 = time.perf_counter()
    idx.build(a.rows, batch=16384, ef_construction=a.efc, seed=1)
    idx.sync()
    log(f"built {a.rows} rows in {time.perf_counter() - t0:.1f} s")
    L, h = idx.L, idx.h
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    res = {"rows": a.rows, "dim": dim, "metric": "cosine", "corpus": "clustered-4096 + 0.3*N(0,1), L2-normalised", "m": 16, "ef_construction": a.efc,
           "queries": B, "ef": ef, "reps": a.reps, "warmup": a.warmup, "host_buffers": "pageable", "host_threads": [1, a.threads], "k": {}}
    for k in a.ks:
        o = [(np.zeros((B, k), np.uint32), np.zeros((B, k), np.float32), np.zeros(B, np.uint32), np.zeros(B, CONSENSUS_DTYPE), np.zeros((B, k), np.float64))
             for _ in range(3)]
        rows = np.zeros((B * k, dim), dtype=np.float32)
        found = np.zeros(B * k, dtype=np.uint8)

        def timed(fn, *args):
            t0 = time.perf_counter()
            rc = fn(*args)
            dt = time.perf_counter() - t0
            assert rc == 0, rc
            return dt

        belief = lambda: timed(L.kdb_belief_batch, h, p(Q), B, k, ef, None, None, 0, p(o[0][0]), p(o[0][1]), p(o[0][2]), p(o[0][3]), p(o[0][4]))
        search = lambda j: timed(L.kdb_search_batch, h, p(Q), B, k, ef, None, 0, p(o[j][0]), p(o[j][1]), p(o[j][2]))
        consensus = lambda: timed(L.kdb_consensus_batch, h, p(o[1][0]), p(o[1][2]), B, k, p(Q), None, 0, p(o[1][3]), p(o[1][4]), None, None)
        decode = lambda: timed(L.kdb_index_decode_rows, h, p(o[2][0]), B * k, p(rows), p(found))
        host = lambda th: timed(shim.consensus_host_many, p(rows), p(o[2][2]), B, k, dim, p(Q), th, p(o[2][3]), p(o[2][4]))
        for _ in range(max(a.warmup, 1)):
            belief()
            search(1)
            consensus()
            search(2)
            decode()
            host(a.threads)
        same = all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(o[0], o[1]))
        assert same, "kdb_belief_batch and kdb_search_batch + kdb_consensus_batch disagree"
        assert found.reshape(B, k)[np.arange(k)[None, :] < o[2][2][:, None]].all()      # no deleted rows here: rows are packed per list
        full = o[2][2] == k
        d_var = float(np.max(np.abs(o[2][3]["variance"][full] - o[1][3]["variance"][full])))
        d_sim = float(np.max(np.abs(o[2][4][full] - o[1][4][full])))
        d_score = float(np.max(np.abs(o[2][3]["score"][full] - o[1][3]["score"][full])))
        log(f"k {k}: device ways equal bit for bit; host vs device max |d variance| {d_var:.3g}, |d similarity| {d_sim:.3g}, |d score| {d_score:.3g}; "
            f"lists with all k results {int(full.sum())} of {B}")
        assert d_var <= 2.0 ** -46 and d_sim <= 2.0 ** -46
        t = {n: [] for n in ("belief", "search_b", "consensus", "search_c", "decode", "host1", "hostN")}
        for _ in range(a.reps):
            t["belief"].append(belief())
            t["search_b"].append(search(1))
            t["consensus"].append(consensus())
            t["search_c"].append(search(2))
            t["decode"].append(decode())
            t["host1"].append(host(1))
            t["hostN"].append(host(a.threads))
        # the kernel alone: device buffers, events
        d_ids = torch.from_numpy(o[1][0].view(np.int32)).to(dev)
        d_cnt = torch.from_numpy(o[1][2].view(np.int32)).to(dev)
        d_q = torch.from_numpy(Q).to(dev)
        d_out = torch.zeros((B, 32), dtype=torch.uint8, device=dev)
        d_sim_t = torch.zeros((B, k), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        st = torch.cuda.Stream()  # a stream of its own: the library runs the kernel on the stream it is handed, the events bracket it there
        kt = []
        for i in range(a.reps + a.warmup):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            idx.consensus_dev(d_ids, d_out, d_cnt, d_q, None, d_sim_t, stream=st.cuda_stream)
            e1.record(st)
            e1.synchronize()
            if i >= a.warmup:
                kt.append(e0.elapsed_time(e1) * 1e-3)
        ans = B * k * 8 + B * 4
        sc = [x + y for x, y in zip(t["search_b"], t["consensus"])]
        h1 = [x + y + z for x, y, z in zip(t["search_c"], t["decode"], t["host1"])]
        hn = [x + y + z for x, y, z in zip(t["search_c"], t["decode"], t["hostN"])]
        med = lambda x: float(np.median(x))
        res["k"][str(k)] = {
            "belief": dict(ms(t["belief"]), bytes_to_device=B * dim * 4, bytes_to_host=ans + B * 32 + B * k * 8),
            "search_consensus": dict(ms(sc), search=ms(t["search_b"]), consensus=ms(t["consensus"]), bytes_to_device=B * dim * 4 + B * k * 4 + B * 4 + B * dim * 4,
                                     bytes_to_host=ans + B * 32 + B * k * 8),
            "host_1_thread": dict(ms(h1), search=ms(t["search_c"]), decode_rows=ms(t["decode"]), consensus_host=ms(t["host1"]),
                                  bytes_to_device=B * dim * 4 + B * k * 4, bytes_to_host=ans + B * k * dim * 4 + B * k),
            f"host_{a.threads}_threads": dict(ms(hn), consensus_host=ms(t["hostN"])),
            "consensus_kernel": ms(kt),
            "device_ways_equal_bit_for_bit": bool(same), "host_vs_device_max_abs": {"variance": d_var, "similarity": d_sim, "score": d_score},
            "belief_over_host_1_thread": round(med(h1) / med(t["belief"]), 3), f"belief_over_host_{a.threads}_threads": round(med(hn) / med(t["belief"]), 3),
            "search_consensus_over_host_1_thread": round(med(h1) / med(sc), 3), f"search_consensus_over_host_{a.threads}_threads": round(med(hn) / med(sc), 3),
        }
        log(json.dumps(res["k"][str(k)]))
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--efc", type=int, default=200)
    ap.add_argument("--queries", type=int, default=4096)
    ap.add_argument("--ks", type=int, nargs="+", default=[10, 50])
    ap.add_argument("--ef", type=int, default=100)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--reps", type=int, default=31)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "consensus_probe.json"))
    ap.add_argument("--step", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.step == "measure":
        return step_measure(a)
    cmd = [sys.executable, os.path.abspath(__file__), "--step", "measure", "--ks"] + [str(k) for k in a.ks]
    for key in ("rows", "dim", "efc", "queries", "ef", "threads", "reps", "warmup"):
        cmd += ["--" + key, str(getattr(a, key))]
    log("step measure, limit 900 s")
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT)
    sys.stderr.write(p.stderr[-6000:])
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
