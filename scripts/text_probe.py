"""BM25 text search and the hybrid request on a synthetic corpus: --docs documents (1M) of --doc-tokens tokens drawn from a Zipf
vocabulary of --vocab words; queries of 3-5 tokens drawn from the same law, so common words occur in them.

  leg 1  kdb_text_search_batch at B = 1, 64, 4096 (host pointers, pageable numpy buffers, k = 10);
  leg 2  the same queries through `host_bm25`: the restatement in numpy on the host -- a union of posting arrays, the term sum in
         query order, a sort.  It stands for the host path the call replaces; it is NOT the Go binary (no map of maps, no GC);
  leg 3  bm25_topk_kernel alone at B = 4096 on device buffers: (8 x postings read + 4 x touched documents) / time, beside the
         streaming ceiling kdb_probe_stream measures in the same run;
  leg 4  kdb_hybrid_search_batch against kdb_search_batch + read-back + host_bm25 + the fusion in Python on the same requests, over a
         --rows x --dim cosine index built on the GPU whose ids are the first --rows documents.

The legs ALTERNATE in one process, --reps times after --warmup rounds; medians, and the spread as (min, max).  The host legs run on at
most --host-queries queries per round (their time per query is what is reported).  Before anything is timed the device call must
equal host_bm25 bit for bit on the first queries.

--split measures one query on many workgroups instead (split_probe, below): this tree against a built checkout of the parent commit,
call by call, then the forced part counts and the posting counts from which splitting pays.

usage: python scripts/text_probe.py [--docs N] [--out profiles/text_probe.json] [--split [--parent-tree DIR]]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def log(*a):
    print("[text_probe]", *a, file=sys.stderr, flush=True)


def ms(x, per=1):
    x = np.asarray(x) * 1e3 / per
    return {"median_ms": round(float(np.median(x)), 5), "min_ms": round(float(x.min()), 5), "max_ms": round(float(x.max()), 5)}


def make_corpus(a, rng):
    p = 1.0 / np.arange(1, a.vocab + 1) ** a.zipf
    cdf = np.cumsum(p / p.sum())
    draw = lambda n: np.minimum(np.searchsorted(cdf, rng.random(n)), a.vocab - 1).astype(np.uint64)
    doc = np.repeat(np.arange(1, a.docs + 1, dtype=np.uint64), a.doc_tokens)
    pair, tf = np.unique(draw(doc.size) * np.uint64(a.docs + 1) + doc, return_counts=True)  # sorted by (token, document)
    tok = (pair // np.uint64(a.docs + 1)).astype(np.int64)
    post_off = np.zeros(a.vocab + 1, dtype=np.uint64)
    post_off[1:] = np.cumsum(np.bincount(tok, minlength=a.vocab))
    doc_len = np.full(a.docs + 1, a.doc_tokens, dtype=np.uint32)
    doc_len[0] = 0
    queries = [draw(int(n)).astype(np.uint32).tolist() for n in rng.integers(3, 6, a.queries)]
    return post_off, (pair % np.uint64(a.docs + 1)).astype(np.uint32), tf.astype(np.uint32), doc_len, queries


def host_bm25(snap, idf, query, k):
    """FindIDsByTextSearch in numpy: (ids, scores) of the first k by (score descending, id ascending), max, candidates"""
    lists = [(int(snap.post_off[t]), int(snap.post_off[t + 1])) for t in query]
    docs = np.unique(np.concatenate([snap.post_doc[lo:hi] for lo, hi in lists])) if lists else np.zeros(0, np.uint32)
    score = np.zeros(docs.size)
    norm = 1.2 * (0.25 + 0.75 * (snap.doc_len[docs] / snap.avg_len))
    for t, (lo, hi) in zip(query, lists):
        at = np.searchsorted(docs, snap.post_doc[lo:hi])
        tf = snap.post_tf[lo:hi].astype(np.float64)
        score[at] = score[at] + idf[t] * ((tf * 2.2) / (tf + norm[at]))
    order = np.lexsort((docs, -score))[:k]
    return docs[order], score[order], (score.max() if docs.size else 0.0), docs.size


def split_worker(a):
    """--worker: the corpus on the device of the tree given by --tree; then one timed kdb_text_search_batch per request line
    {"q": queries, "split": KDB_TEXT_SPLIT or null} -> {"s": seconds, "ncand": candidates, "digest": of the answer}"""
    import hashlib
    sys.path.insert(0, a.tree)
    import kektordb_amd as K
    post_off, post_doc, post_tf, doc_len, _ = make_corpus(a, np.random.default_rng(5))
    snap = K.TextIndex.from_arrays(post_off, post_doc, post_tf, doc_len, a.docs, float(a.doc_tokens))
    df = np.diff(post_off.astype(np.int64)).astype(np.float64)
    idx = K.HipIndex(16, K.L2, K.F32, capacity=a.docs)
    idx.upload_rows(np.zeros((a.docs, 16), dtype=np.float32), 1)
    idx.set_count(a.docs)
    idx.set_text(0, snap, np.log(1 + (a.docs - df + 0.5) / (df + 0.5)))
    print(json.dumps({"ready": True, "stream_GBps": round(idx.probe_stream(), 1)}), flush=True)
    for line in sys.stdin:
        req = json.loads(line)
        os.environ.pop("KDB_TEXT_SPLIT", None)
        if req["split"] is not None:
            os.environ["KDB_TEXT_SPLIT"] = str(req["split"])
        t0 = time.perf_counter()
        out = idx.text_search(0, req["q"], a.k)
        dt = time.perf_counter() - t0
        print(json.dumps({"s": dt, "ncand": int(out[4].astype(np.int64).sum()), "digest": hashlib.sha1(b"".join(x.tobytes() for x in out)).hexdigest()[:12]}), flush=True)


def split_probe(a):
    """--split: one query on many workgroups.  Workers of this tree and, with --parent-tree, of a built checkout of the parent commit
    hold the same corpus; the driver sends ONE call at a time, so legs alternate call by call in one session on one box.
      table 1  B = 1, 8, 64, 4096: this tree against the parent (or, without one, against KDB_TEXT_SPLIT=0), factors, spreads,
               posting bytes per second beside the streaming ceiling;
      table 2  B = 1, the first query, forced 32 / 64 / 128 / 245 / 512 parts;
      table 3  B = 1, one token per query, lists of growing length: the fastest forced setting of table 2 against KDB_TEXT_SPLIT=0."""
    import subprocess
    rng = np.random.default_rng(5)
    post_off, _, _, _, queries = make_corpus(a, rng)
    df = np.diff(post_off.astype(np.int64))
    base = [sys.executable, os.path.abspath(__file__), "--worker", "--docs", str(a.docs), "--doc-tokens", str(a.doc_tokens), "--vocab", str(a.vocab),
            "--zipf", str(a.zipf), "--queries", str(a.queries), "--k", str(a.k)]
    trees = {"this": ROOT, **({"parent": a.parent_tree} if a.parent_tree else {})}
    procs = {n: subprocess.Popen(base + ["--tree", t], stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, env={k: v for k, v in os.environ.items() if k != "KDB_TEXT_SPLIT"}) for n, t in trees.items()}
    ceiling = {n: json.loads(p.stdout.readline())["stream_GBps"] for n, p in procs.items()}
    log("workers ready, streaming ceilings", ceiling)

    def call(who, q, split=None):
        procs[who].stdin.write(json.dumps({"q": q, "split": split}) + "\n")
        procs[who].stdin.flush()
        return json.loads(procs[who].stdout.readline())

    def race(legs, q):  # legs: {name: (worker, KDB_TEXT_SPLIT)}; alternating; every leg must give the same answer
        times, last = {n: [] for n in legs}, {}
        for r in range(a.warmup + a.reps):
            for n, (who, split) in legs.items():
                last[n] = call(who, q, split)
                if r >= a.warmup:
                    times[n].append(last[n]["s"])
        assert len({v["digest"] for v in last.values()}) == 1, last
        return {n: ms(t) for n, t in times.items()}, next(iter(last.values()))["ncand"]

    other = ("parent", None) if a.parent_tree else ("this", 0)
    out = {"docs": a.docs, "k": a.k, "reps": a.reps, "against": "parent commit" if a.parent_tree else "KDB_TEXT_SPLIT=0", "stream_ceiling_GBps": ceiling["this"], "by_B": {}}
    for B in (1, 8, 64, a.queries):
        q = queries[:B]
        t, ncand = race({"this": ("this", None), "other": other}, q)
        byts = 8 * int(sum(int(df[tok]) for x in q for tok in x)) + 4 * ncand
        out["by_B"][f"B{B}"] = {**t, "factor": round(t["other"]["median_ms"] / t["this"]["median_ms"], 3),
                               "posting_GBps": round(byts / t["this"]["median_ms"] / 1e6, 2), "of_ceiling": round(byts / t["this"]["median_ms"] / 1e6 / ceiling["this"], 4)}
        log(f"B{B}", out["by_B"][f"B{B}"])
    t, _ = race({f"parts{n}": ("this", n) for n in (32, 64, 128, 245, 512)}, queries[:1])
    out["by_parts_B1"] = t
    best = int(min(t, key=lambda n: t[n]["median_ms"])[5:])
    log("parts", t, "fastest", best)
    out["by_postings_B1"] = {}
    for want in [1 << e for e in range(0, 20)] + [int(df.max())]:
        tok = int(np.argmin(np.abs(df - want)))
        t, _ = race({"split": ("this", best), "unsplit": ("this", 0)}, [[tok]])
        out["by_postings_B1"][str(int(df[tok]))] = {n: v["median_ms"] for n, v in t.items()}
        log("postings", int(df[tok]), out["by_postings_B1"][str(int(df[tok]))])
    for p in procs.values():
        p.stdin.close()
        p.wait()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--split", action="store_true", help="measure the split sweep only; merged into --out under 'split'")
    ap.add_argument("--parent-tree", default=None, help="--split: a built checkout of the parent commit to race against")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=ROOT, help=argparse.SUPPRESS)
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--doc-tokens", type=int, default=40)
    ap.add_argument("--vocab", type=int, default=50_000)
    ap.add_argument("--zipf", type=float, default=1.1)
    ap.add_argument("--queries", type=int, default=4096)
    ap.add_argument("--host-queries", type=int, default=16)
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--ef", type=int, default=100)
    ap.add_argument("--reps", type=int, default=31)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "text_probe.json"))
    a = ap.parse_args()
    if a.worker:
        return split_worker(a)
    if a.split:
        old = {}
        if os.path.exists(a.out):
            with open(a.out) as f:
                old = json.load(f)
        old["split"] = split_probe(a)
        with open(a.out, "w") as f:
            json.dump(old, f, indent=1)
        print(json.dumps(old["split"]))
        return
    import torch
    import kektordb_amd as K
    from kektordb_amd.index import pack_token_queries
    rng = np.random.default_rng(5)
    t0 = time.perf_counter()
    post_off, post_doc, post_tf, doc_len, queries = make_corpus(a, rng)
    snap = K.TextIndex.from_arrays(post_off, post_doc, post_tf, doc_len, a.docs, float(a.doc_tokens))
    df = np.diff(post_off.astype(np.int64)).astype(np.float64)
    idf = np.log(1 + (a.docs - df + 0.5) / (df + 0.5))
    log(f"corpus: {a.docs} documents, {post_doc.size} postings, longest list {int(df.max())}, {time.perf_counter() - t0:.1f} s")
    X = rng.standard_normal((a.rows, a.dim)).astype(np.float32)
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    idx = K.HipIndex(a.dim, K.COSINE, K.F32, 16, 100, capacity=a.docs)
    idx.upload_rows(X, 1)
    idx.build(a.rows, batch=16384, ef_construction=100, seed=1)
    idx.set_text(0, snap, idf)
    Q = (X[rng.choice(a.rows, a.queries)] + 0.05 * rng.standard_normal((a.queries, a.dim))).astype(np.float32)
    k, hq = a.k, min(a.host_queries, a.queries)
    ids, score, cnt, mx, nc = idx.text_search(0, queries[:hq], k)
    for b in range(hq):  # the gate: the device call is the restatement, bit for bit
        hi, hs, hm, hn = host_bm25(snap, idf, queries[b], k)
        assert ids[b, :len(hi)].tolist() == hi.tolist() and score[b, :len(hs)].view(np.uint64).tolist() == hs.view(np.uint64).tolist(), b
        assert (int(nc[b]), mx[b]) == (hn, hm), b

    def host_hybrid(b0, b1, alpha=0.5):
        v_ids, v_dist, v_cnt = idx.search_batch(Q[b0:b1], k, a.ef)
        for b in range(b0, b1):
            ti, ts, tm, _ = host_bm25(snap, idf, queries[b], 1 << 30)
            fused = {int(d): alpha / (1.0 + (1.0 - float(x))) for d, x in zip(v_ids[b - b0, :v_cnt[b - b0]], v_dist[b - b0])}
            for d, s in zip(ti.tolist(), (ts / tm if tm > 0 else ts).tolist()):
                fused[d] = fused.get(d, 0.0) + (1 - alpha) * s
            sorted(fused.items(), key=lambda e: (-e[1], e[0]))[:k]

    tok, nt = pack_token_queries(queries)
    dev = lambda x: torch.from_numpy(x.view(np.int32)).cuda()
    d_tok, d_nt = dev(tok), dev(nt)
    d_ids, d_cnt, d_nc = (torch.zeros(s, dtype=torch.int32, device="cuda") for s in ((a.queries, k), a.queries, a.queries))
    d_score = torch.zeros((a.queries, k), dtype=torch.float64, device="cuda")

    def kernel_only():
        idx.text_search_dev(0, d_tok, d_nt, k, d_ids, d_score, d_cnt, None, d_nc)
        idx.sync()

    sizes = sorted({1, min(8, a.queries), min(64, a.queries), a.queries})
    legs = {f"text_B{B}": (lambda B=B: idx.text_search(0, queries[:B], k)) for B in sizes}
    legs["host_bm25"] = lambda: [host_bm25(snap, idf, q, k) for q in queries[:hq]]
    legs["kernel"] = kernel_only
    legs["hybrid"] = lambda: idx.hybrid_search(Q, k, a.ef, 0, queries, 0.5)
    legs["hybrid_host"] = lambda: host_hybrid(0, hq)
    times = {name: [] for name in legs}
    for r in range(a.warmup + a.reps):
        for name, f in legs.items():
            t0 = time.perf_counter()
            f()
            if r >= a.warmup:
                times[name].append(time.perf_counter() - t0)
    postings = int(sum(int(post_off[t + 1] - post_off[t]) for q in queries for t in q))
    touched = int(d_nc.cpu().numpy().view(np.uint32).astype(np.int64).sum())
    kern_s = float(np.median(times["kernel"]))
    out = {"docs": a.docs, "postings": int(post_doc.size), "longest_list": int(df.max()), "k": k, "reps": a.reps,
           "text_search": {f"B{B}": ms(times[f"text_B{B}"]) for B in sizes},
           "host_bm25_numpy_per_query": ms(times["host_bm25"], hq),
           "device_per_query_at_max_B": ms(times[f"text_B{a.queries}"], a.queries),
           "kernel": {**ms(times["kernel"]), "postings_read": postings, "touched_docs": touched,
                      "posting_GBps": round((8 * postings + 4 * touched) / kern_s / 1e9, 2), "stream_ceiling_GBps": round(idx.probe_stream(), 1)},
           "hybrid": {"rows": a.rows, "dim": a.dim, "ef": a.ef, "device_per_query": ms(times["hybrid"], a.queries),
                      "search_plus_host_bm25_plus_host_fusion_per_query": ms(times["hybrid_host"], hq)}}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
