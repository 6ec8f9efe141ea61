"""Search by stored id on the headline corpus (1M x 768 cosine, clustered, m 16, efConstruction 200): one page of ids through
kdb_search_by_id against the same work done the way it had to be done before -- the rows read back (kdb_index_download_rows, the
mirror's VGetMany) and handed to kdb_search_batch as queries.  Host pointers on both sides, pageable numpy buffers, the C calls
themselves timed (a host clock around calls that end in a stream synchronise).

  * by_id             kdb_search_by_id(ids): 4 bytes per query go in, the answers come out;
  * rows_then_search  kdb_index_download_rows(page) + kdb_search_batch(those rows): dim x 4 bytes per query come out and go in again;
  * search_only       kdb_search_batch alone on rows that are already in host memory (what the copies of the second call cost).

The page is --queries consecutive ids (VGetIDsByCursor hands out ids in order; one kdb_index_download_rows call reads them).  The
legs ALTERNATE inside one process, --reps times after --warmup rounds; medians, and the spread as (min, max).  The answers of the
two ways are compared before anything is timed: they must be equal bit for bit.  The measurement runs in a child process under
its own time limit; a step that fails ends the probe.

usage: python scripts/by_id_probe.py [--rows N] [--queries B] [--out profiles/by_id_probe.json]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def log(*a):
    print("[by_id_probe]", *a, file=sys.stderr, flush=True)


def ms(x):
    x = np.asarray(x) * 1e3
    return {"median_ms": round(float(np.median(x)), 4), "min_ms": round(float(x.min()), 4), "max_ms": round(float(x.max()), 4)}


def step_measure(a):
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
    del X
    t0 = time.perf_counter()
    idx.build(a.rows, batch=16384, ef_construction=a.efc, seed=1)
    idx.sync()
    log(f"built {a.rows} rows in {time.perf_counter() - t0:.1f} s")
    B, k, ef, dim = a.queries, a.k, a.ef, a.dim
    first = (a.rows - B) // 2 + 1
    ids = np.arange(first, first + B, dtype=np.uint32)
    rows = np.zeros((B, dim), dtype=np.float32)
    out = [(np.zeros((B, k), np.uint32), np.zeros((B, k), np.float32), np.zeros(B, np.uint32)) for _ in range(2)]
    L, h = idx.L, idx.h
    p = lambda x: x.ctypes.data_as(C.c_void_p)

    def by_id():
        t0 = time.perf_counter()
        rc = L.kdb_search_by_id(h, p(ids), B, k, ef, None, 0, p(out[0][0]), p(out[0][1]), p(out[0][2]))
        dt = time.perf_counter() - t0
        assert rc == 0, rc
        return dt

    def download():
        t0 = time.perf_counter()
        rc = L.kdb_index_download_rows(h, first, B, p(rows))
        dt = time.perf_counter() - t0
        assert rc == 0, rc
        return dt

    def search():
        t0 = time.perf_counter()
        rc = L.kdb_search_batch(h, p(rows), B, k, ef, None, 0, p(out[1][0]), p(out[1][1]), p(out[1][2]))
        dt = time.perf_counter() - t0
        assert rc == 0, rc
        return dt

    # same answers first (also the warm-up of both shapes: code objects, scratch, the walk planes)
    for _ in range(max(a.warmup, 1)):
        by_id()
        download()
        search()
    same = all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(out[0], out[1]))
    self_first = float(np.mean(out[0][0][:, 0] == ids))
    log(f"answers equal bit for bit: {same}; a stored row ranks itself first in {self_first:.4f} of the page")
    assert same, "kdb_search_by_id and kdb_search_batch on the downloaded rows disagree"
    t_id, t_dl, t_s = [], [], []
    for _ in range(a.reps):  # alternating: by id, then the old way
        t_id.append(by_id())
        t_dl.append(download())
        t_s.append(search())
    t_old = [x + y for x, y in zip(t_dl, t_s)]
    ans = B * k * 8 + B * 4
    res = {"rows": a.rows, "dim": dim, "metric": "cosine", "corpus": "clustered-4096 + 0.3*N(0,1), L2-normalised", "m": 16, "ef_construction": a.efc,
           "queries": B, "k": k, "ef": ef, "page": [int(first), int(first + B - 1)], "reps": a.reps, "warmup": a.warmup, "host_buffers": "pageable",
           "answers_equal_bit_for_bit": bool(same), "self_ranks_first": round(self_first, 4),
           "by_id": dict(ms(t_id), qps=round(B / float(np.median(t_id)), 1), bytes_to_device=B * 4, bytes_to_host=ans),
           "rows_then_search": dict(ms(t_old), qps=round(B / float(np.median(t_old)), 1), bytes_to_device=B * dim * 4, bytes_to_host=B * dim * 4 + ans,
                                    download=ms(t_dl), search=ms(t_s)),
           "search_only": dict(ms(t_s), qps=round(B / float(np.median(t_s)), 1), bytes_to_device=B * dim * 4, bytes_to_host=ans)}
    res["by_id_over_rows_then_search"] = round(float(np.median(t_old)) / float(np.median(t_id)), 3)
    res["by_id_over_search_only"] = round(float(np.median(t_s)) / float(np.median(t_id)), 3)
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--efc", type=int, default=200)
    ap.add_argument("--queries", type=int, default=32768)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--ef", type=int, default=60)
    ap.add_argument("--reps", type=int, default=31)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "by_id_probe.json"))
    ap.add_argument("--step", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.step == "measure":
        return step_measure(a)
    cmd = [sys.executable, os.path.abspath(__file__), "--step", "measure"]
    for key in ("rows", "dim", "efc", "queries", "k", "ef", "reps", "warmup"):
        cmd += ["--" + key, str(getattr(a, key))]
    log("step measure, limit 600 s")
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    sys.stderr.write(p.stderr[-4000:])
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
