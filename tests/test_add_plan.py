"""kdb_index_add without a GPU: the host-side plan (kektordb_amd/csrc/kdb_add_plan.h) -- the capped level of every node of a
call and the entry point / maxLevel it finds -- against the oracle's sequential Add (hnsw_index.go:472-809, :2620-2623), in a
stand-alone C++ program built with AddressSanitizer and UBSan; and the entry point's presence in header, library and binding."""
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def record(O, prior, asked, seed):
    """`prior` forced levels inserted first (the state the call finds), then `asked`: -> the case's lines"""
    dim = 4
    rng = np.random.default_rng(seed)
    orc = O.OracleIndex(dim, O.L2, O.F32, 4, 8, seed=1)
    for lv in prior:
        orc.add(rng.random(dim, dtype=np.float32), level=int(lv))
    head = f"{orc.entry} {orc.max_level} {orc.count + 1} {len(asked)}"
    lines = []
    for lv in asked:
        nid = orc.add(rng.random(dim, dtype=np.float32), level=int(lv))
        kept = int(orc.export_graph().levels[nid])
        lines.append(f"{int(lv)} {kept} {orc.entry} {orc.max_level}")
    return [head] + lines


def test_add_plan_matches_oracle(oracle, tmp_path):
    O = oracle
    rng = np.random.default_rng(5)
    ml = 1.0 / np.log(4)
    usual = np.minimum(np.floor(-np.log(1.0 - rng.random(60)) * ml), 6).astype(int)
    cases = [
        record(O, [], usual, 1),                                            # starts empty, the usual draw
        record(O, [], [0, 1, 0, 2, 2, 3, 0, 1, 4, 0, 5, 5, 6, 0], 2),       # raises maxLevel several times
        record(O, [], [0, 6, 6, 0, 250, 3, 255, 1, 0, 9], 3),               # levels far above maxLevel + 1: the cap
        record(O, [], [0], 4),                                              # n = 1, the first node of an empty graph
        record(O, [], [5], 5),                                              # ... asking for a level: capped at 0
        record(O, [0, 1, 0, 2, 0], [3], 6),                                 # n = 1, raises the top of a graph
        record(O, [0, 1, 0, 2, 0], [1], 7),                                 # n = 1, below the top
        record(O, list(usual[:30]), list(usual[30:]) + [6, 6, 6], 8),       # continues a graph
        record(O, [2, 0], [], 9),                                           # n = 0
    ]
    path = tmp_path / "cases.txt"
    path.write_text("\n".join([str(len(cases))] + [l for c in cases for l in c]) + "\n")
    exe = str(tmp_path / "add_plan_test")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Werror",
           "-I", os.path.join(ROOT, "kektordb_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "add_plan_test.cpp"), "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.startswith(f"ok {len(cases)} cases"), r.stdout
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]


def test_kdb_index_add_declared_exported_bound():
    import kektordb_amd
    from kektordb_amd import _lib
    kektordb_amd.build_library()
    txt = open(os.path.join(ROOT, "include", "kektor_hip.h")).read()
    assert re.search(r"KDB_API\s+int\s+kdb_index_add\s*\(", txt)
    assert "kdb_add_params" in txt and "kdb_add_stats" in txt and "hnsw_index.go:472-809" in txt
    out = subprocess.run(["nm", "-D", "--defined-only", kektordb_amd.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert any(l.split()[-1] == "kdb_index_add" and " T " in l for l in out.splitlines())
    assert "kdb_index_add" in _lib.ABI_SYMBOLS
    assert _lib.load().kdb_index_add.argtypes is not None
    assert [f for f, _ in _lib.AddStats._fields_] == ["nodes_added", "forward_lists", "reverse_appended", "reverse_pruned", "tied_nodes",
                                                     "reverse_skipped", "entry", "max_level"]
    assert hasattr(kektordb_amd.HipIndex, "add")
