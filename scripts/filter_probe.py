"""Allow lists built on the device (kdb_filter_eval_dev, kdb_search_filtered) on the table of bench.py's config 5: 10M ids, one code
column of 100 categories, 100 programs `cat = c`.  Writes profiles/filter_probe.json.

  (a) against the host path it replaces, on the same box: numpy dense_bitset for the 100 lists (the ids of every category are handed
      over ready made, as roaring would) plus their copy to the device, against kdb_filter_eval_dev.  Both legs end with the lists
      resident in HBM and the device idle.  Legs ALTERNATE, --reps times after one warm-up round; medians, spread as (min, max).
  (b) against the streaming ceiling: the kernel's algorithmic bytes -- every column the programs read, once, plus P x words written
      -- over its HIP-event time, as a fraction of what kdb_probe_stream measures in the same run on the same index.
  (c) against the lists-resident search figure: config 5 as written (--rows x 1536 cosine, --queries queries each with its own
      random category, k = 10) through kdb_search_filtered -- host pointers, lists made inside the timed region -- next to ONE
      kdb_flat_scan_groups_dev call on lists that are already resident (what bench.py's configs[4] times), same index, same run.
      The two answers are compared first.
  (d) a `!=` program: `_is_historical != 'true'` with 1 % of the ids marked, one list.

(a), (b) and (d) run on a 16-column index (the filter reads no row); (c) needs the full table and is skipped with --no-search.
usage: python scripts/filter_probe.py [--rows N] [--queries B] [--reps R] [--no-search] [--out profiles/filter_probe.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


WAITS_FOR = ("not HBM: as written the kernel reads the column once per chunk of 32 programs (4 chunks here: 160 MB) and writes 125 MB, "
             "which this device streams in well under 0.1 ms; the time goes to the term loop (per tile and program: offsets and terms "
             "through the scalar cache, 16 LDS reads and compares per lane, 16 ballots) and to one atomic add per (tile, program) on 100 "
             "adjacent counters (977 k of them); which of the two dominates has not been separated")


def log(*a):
    print("[filter_probe]", *a, file=sys.stderr, flush=True)


def ms(x):
    x = np.asarray(x) * 1e3
    return {"median_ms": round(float(np.median(x)), 4), "min_ms": round(float(x.min()), 4), "max_ms": round(float(x.max()), 4), "n": int(x.size)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=31)
    ap.add_argument("--ncat", type=int, default=100)
    ap.add_argument("--no-search", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "filter_probe.json"))
    a = ap.parse_args()
    import torch
    import kektordb_amd as K
    from kektordb_amd.index import COL_CODE, FOP_CODE_EQ, FT_END_BLOCK, FT_NOT, TERM_DTYPE, dense_bitset
    dev = torch.device("cuda:0")
    n, P = a.rows, a.ncat
    words = (n >> 6) + 1
    rng = np.random.default_rng(3)
    out = {"rows": n, "programs": P, "words_per_list": words, "list_bytes": words * 8}

    # ---- (a), (b), (d): the columns alone
    idx = K.HipIndex(16, K.L2, K.F32, 16, 200, capacity=n)
    idx.set_count(n)
    cat = rng.integers(0, P, n + 1).astype(np.uint32) + 1          # codes 1..P, entry 0 unused
    idx.set_column(0, COL_CODE, cat[1:], 1)
    hist = (rng.random(n + 1) < 0.01).astype(np.uint32)            # 1 = "true", 0 = no value
    idx.set_column(1, COL_CODE, hist[1:], 1)
    progs = [np.array([(FOP_CODE_EQ, FT_END_BLOCK, 0, c + 1, 0.0)], dtype=TERM_DTYPE) for c in range(P)]
    ids_of = [np.nonzero(cat[1:] == c + 1)[0].astype(np.uint32) + 1 for c in range(P)]
    d_lists = torch.zeros((P, words), dtype=torch.int64, device=dev)
    d_card = torch.zeros(P, dtype=torch.int32, device=dev)
    side = torch.cuda.Stream()

    def host_path():
        t0 = time.perf_counter()
        lists = np.stack([dense_bitset(ids_of[c], n) for c in range(P)])
        t1 = time.perf_counter()
        d = torch.from_numpy(lists.view(np.int64)).to(dev)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, t1 - t0, d

    def device_path():
        t0 = time.perf_counter()
        idx.filter_eval_dev(progs, d_lists, d_card, stream=side.cuda_stream)
        side.synchronize()
        return time.perf_counter() - t0

    _, _, ref = host_path()
    device_path()
    assert torch.equal(ref, d_lists), "device lists differ from dense_bitset's"
    assert d_card.cpu().numpy().tolist() == [int(x.size) for x in ids_of]
    del ref
    th, tb, td = [], [], []
    for r in range(a.reps):
        h, b, d = host_path()
        del d
        th.append(h)
        tb.append(b)
        td.append(device_path())
    out["a_host_path_vs_device"] = {
        "host_path": ms(th), "host_path_bitsets_only": ms(tb), "filter_eval_dev": ms(td),
        "speedup_of_medians": round(float(np.median(th) / np.median(td)), 1),
        "definition": f"host: numpy dense_bitset x {P} + stack + one copy to the device, synchronised; device: kdb_filter_eval_dev "
                      f"({P} programs cat = c, lists and cardinalities in HBM), synchronised; legs alternate"}
    log("(a)", out["a_host_path_vs_device"])

    def event_ms(programs, lists, card, reps):
        ts = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(side):
                e0.record()
            idx.filter_eval_dev(programs, lists, card, stream=side.cuda_stream)
            with torch.cuda.stream(side):
                e1.record()
            side.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e-3)
        return ts

    tk = event_ms(progs, d_lists, d_card, a.reps)
    alg = (n + 1) * 4 + P * words * 8
    stream_gbps = idx.probe_stream()
    gbps = alg / float(np.median(tk)) / 1e9
    out["b_streaming_ceiling"] = {
        "hip_event": ms(tk), "algorithmic_bytes": int(alg), "bytes_definition": "the code column once ((rows + 1) x 4) + programs x words x 8 written",
        "achieved_gbps": round(gbps, 1), "kdb_probe_stream_gbps": round(stream_gbps, 1), "frac_of_measured_stream": round(gbps / stream_gbps, 4),
        "bytes_read_by_the_kernel_as_written": int(-(-P // 32) * ((n + 1) * 4 + (n >> 3))),
        "waits_for": WAITS_FOR}
    log("(b)", out["b_streaming_ceiling"])

    ne = [np.array([(FOP_CODE_EQ, FT_NOT | FT_END_BLOCK, 1, 1, 0.0)], dtype=TERM_DTYPE)]
    d_one = torch.zeros((1, words), dtype=torch.int64, device=dev)
    d_c1 = torch.zeros(1, dtype=torch.int32, device=dev)
    tn = event_ms(ne, d_one, d_c1, a.reps)
    assert int(d_c1.cpu().numpy()[0]) == int(n - hist[1:].sum())
    out["d_not_equal_program"] = {"filter": "_is_historical != 'true'", "marked_frac": 0.01, "hip_event": ms(tn), "cardinality": int(d_c1.cpu().numpy()[0])}
    log("(d)", out["d_not_equal_program"])
    idx.close()
    del idx, d_lists, d_one
    torch.cuda.empty_cache()

    # ---- (c): config 5 as written
    if not a.no_search:
        from bench import c5_case, outs
        g = torch.Generator(device=dev)
        g.manual_seed(3)
        nq, k = a.queries, 10
        idx, Q, Qs, cats, offs, allowed, total, d_res = c5_case(K, dev, g, n, nq)
        code = np.zeros(n + 1, dtype=np.uint32)
        for j, c in enumerate(cats):
            code[allowed[int(c)]] = j + 1
        idx.set_column(0, COL_CODE, code[1:], 1)
        progs5 = [np.array([(FOP_CODE_EQ, FT_END_BLOCK, 0, j + 1, 0.0)], dtype=TERM_DTYPE) for j in range(len(cats))]
        # the sorted batch Qs is what the grouped scan takes; query i of it belongs to group j with offs[j] <= i < offs[j + 1]
        poq = np.repeat(np.arange(len(cats)), np.diff(offs.astype(np.int64)))
        Qh = Qs.cpu().numpy()
        o = outs(nq, k, dev)

        def resident():
            t0 = time.perf_counter()
            idx.flat_scan_groups_dev(Qs, k, offs, d_res, *o, max_total_allowed=total)
            idx.sync()
            return time.perf_counter() - t0

        def filtered():
            t0 = time.perf_counter()
            r = idx.search_filtered(Qh, k, 0, progs5, poq, flat_selectivity=0.1)
            return time.perf_counter() - t0, r

        resident()
        _, r = filtered()
        want = o[0].cpu().numpy().view(np.uint32)
        assert np.array_equal(r[0], want) and (r[3] == 1).all(), "kdb_search_filtered differs from the grouped scan on resident lists"
        tr, tf = [], []
        for _ in range(max(3, a.reps // 4)):
            tr.append(resident())
            tf.append(filtered()[0])
        out["c_search_with_lists_inside"] = {
            "workload": f"{n}x1536 cosine k={k}, {nq} queries each with its own random category ({len(cats)} programs)",
            "lists_resident_grouped_scan": ms(tr), "search_filtered_host_pointers": ms(tf),
            "qps_lists_resident": round(nq / float(np.median(tr)), 1), "qps_search_filtered": round(nq / float(np.median(tf)), 1),
            "definition": "lists_resident: one kdb_flat_scan_groups_dev on device queries and lists already in HBM (bench.py configs[4]); "
                          "search_filtered: kdb_search_filtered on host queries -- programs evaluated, cardinalities read back, queries "
                          "uploaded, the same grouped scan, answers copied back -- the whole request"}
        log("(c)", out["c_search_with_lists_inside"])
        idx.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
