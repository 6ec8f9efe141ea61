"""Where the planes walk's time goes on the headline shape (1M x 768 clustered cosine, k = 10, ef 60, 32768 queries per launch;
DESIGN 5.1).  KEKTOR_HIP_LIB selects the build.

    python scripts/dbg/planes_profile.py [--probe]
        kernel ms of the launch (mean / min of 5); --probe: then kdb_probe_gather on this index, whole 3072-byte rows and the
        1536-byte rows of the high walk plane (same kernel, launch shapes and best-of rule)
    python scripts/dbg/planes_profile.py --timers > walks.txt      (timers build, `make dbgs`: the first 64 walks print their cycles)
    python scripts/dbg/planes_profile.py --parse walks.txt
        per level-0 hop: pop, list, visited, rows, insert; the rows phase split into high-plane wait / arithmetic, low-plane wait /
        exact arithmetic; the share of hops with more than 8 new neighbours (two trips)"""
import os
import re
import sys

if "--parse" in sys.argv:
    rows = []
    for line in open(sys.argv[sys.argv.index("--parse") + 1]):
        if not line.startswith("q ") or "level 0: pop" not in line:
            continue
        g = lambda pat: int(re.search(pat, line).group(1))
        r = {"hops": g(r"hops (\d+)"), "total": g(r"total (\d+)"), "upper": g(r"upper-layers (\d+)"), "pop": g(r"pop (\d+)"), "list": g(r"list (\d+)"),
             "visited": g(r"visited (\d+)"), "rows": g(r" rows (\d+)"), "insert": g(r"predict\+post\+insert (\d+)")}
        m = re.search(r"planes (\d+): level-0 hops with new neighbours (\d+), with more than 8 (\d+), trips (\d+), with a low-plane trip (\d+), "
                      r"cycles high-wait (\d+) high-math (\d+) low-wait (\d+) low-math (\d+) not-full (\d+)", line)
        if m:
            r.update(zip(("pl", "eval_hops", "two_trips", "trips", "trips_lo", "hi_wait", "hi_math", "lo_wait", "lo_math", "notfull"), map(int, m.groups())))
        rows.append(r)
    assert rows, "no walk lines"
    n = len(rows)
    tot = lambda k: sum(r.get(k, 0) for r in rows)
    hops = tot("hops")
    print(f"{n} walks, {hops / n:.1f} hops per walk (all levels), {tot('total') / n:.0f} cycles per walk, upper layers {tot('upper') / n:.0f}")
    print("cycles per hop (level-0 cycles over all hops): " + ", ".join(f"{k} {tot(k) / hops:.0f}" for k in ("pop", "list", "visited", "rows", "insert")))
    if tot("eval_hops"):
        eh = tot("eval_hops")
        print(f"level-0 hops with new neighbours {eh / n:.1f} per walk, with more than 8 (two trips or more) {tot('two_trips') / eh:.3f}; "
              f"trips {tot('trips') / n:.1f} per walk, with a low-plane round trip {tot('trips_lo') / max(tot('trips'), 1):.3f}")
        print("rows phase, cycles per hop with new neighbours: " + ", ".join(f"{k} {tot(k) / eh:.0f}" for k in ("hi_wait", "hi_math", "lo_wait", "lo_math", "notfull")))
    sys.exit(0)

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import kektordb_amd as K
import bench as Bm

dev = torch.device("cuda:0")
n, dim, k, ef, B = 1_000_000, 768, 10, 60, 32768
gc = torch.Generator(device=dev)
gc.manual_seed(2)
cent = torch.randn((4096, dim), device=dev, generator=gc)
X = Bm.gen_corpus(n, dim, "clustered", 1000, dev, cent)
Q = Bm.gen_corpus(B, dim, "clustered", 11, dev, cent)
idx = K.HipIndex(dim, K.COSINE, K.F32, 16, 200, capacity=n)
idx.upload_rows(X, 1)
del X
idx.build(n, batch=16384, ef_construction=200, seed=1)
o = Bm.outs(B, k, dev)
sys.stdout.flush()
idx.search_batch_dev(Q, k, ef, *o)
idx.sync()
if "--timers" in sys.argv:
    sys.exit(0)
reps = 5
for _ in range(reps):
    idx.search_batch_dev(Q, k, ef, *o)
idx.sync()
st = idx.launch_stats(reps)
ms = [c["kernel_ms"] for c in st]
print(f"library {os.environ.get('KEKTOR_HIP_LIB', '(default)')}: kernel ms mean {np.mean(ms):.4f} min {np.min(ms):.4f}, "
      f"{np.mean([c['n_dist'] for c in st]) / B:.1f} evaluations and {np.mean([c['n_hops'] for c in st]) / B:.1f} hops per query", flush=True)
if "--probe" in sys.argv:
    whole = idx.probe_gather(6_000_000)
    hi = idx.probe_gather(12_000_000, walk_hi=True)
    print(f"uniform random gather on this index, nothing else running: whole rows ({dim * 4} B) {whole:.0f} GB/s, high walk plane ({dim * 2} B) {hi:.0f} GB/s", flush=True)
