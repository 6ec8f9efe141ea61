"""Index::CompileFilter / EvalFilters / SearchFiltered of the C++ host mirror (include/kektor_hip.hpp): tests/cpp/filter_mirror_test.cpp
compiles with plain g++ against the header and links the shared library.  The documents are those of the reference's own filter tests
(tests/golden/filter_kats.json), the expected ids come from tests/filter_ref.py.  Without a GPU the program checks CompileFilter -- it
needs no device -- and then fails loudly (exit 77); on the GPU the lists, cardinalities, routes and answers must match."""
import json
import os
import subprocess

import numpy as np
import pytest

import filter_ref as R
from test_filter_parse import schema_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def write_cases(path):
    kats = json.load(open(os.path.join(ROOT, "tests", "golden", "filter_kats.json")))
    s = kats["sets"][0]
    docs = {i + 1: d["meta"] for i, d in enumerate(s["docs"])}
    schema, cols = schema_of(docs)
    db = R.MetaDB(docs)
    filters = [c["filter"] for c in s["cases"]] + ["year<2021 OR tag=456 OR name='tech_media'", "nokey!=1", "content = 'apple banana'"]
    n = len(docs)
    out = [str(n), str(len(cols))]
    for slot, col in cols.items():
        f64 = col.dtype == np.float64
        out.append(f"{1 if f64 else 2} {slot}")
        out.append(" ".join(("nan" if np.isnan(v) else repr(float(v))) if f64 else str(int(v)) for v in col[1:]))
    out.append(str(len(schema)))
    for key, ent in schema.items():
        out.append(f"{-1 if ent['f64'] is None else ent['f64']} {-1 if ent['code'] is None else ent['code']} {len(ent['dict'])}")
        out.append(key)
        for text, code in ent["dict"].items():
            out += [str(code), text]
    out.append(str(len(filters)))
    for f in filters:
        want = sorted(db.find_ids(f))
        out += [f, " ".join(map(str, [len(want)] + want))]
    with open(path, "w") as fh:
        fh.write("\n".join(out) + "\n")


def build_exe(tmp_path):
    import kektordb_amd
    kektordb_amd.build_library()
    exe = str(tmp_path / "filter_mirror_test")
    libdir = os.path.dirname(kektordb_amd.LIB_PATH)
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "filter_mirror_test.cpp"), "-L", libdir, "-lkektor_hip",
           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-pthread", "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    return exe


@pytest.mark.skipif(__import__("conftest").HAS_GPU, reason="CPU-only behaviour")
def test_cpp_filter_mirror_compiles_filters_and_fails_loudly_without_gpu(tmp_path):
    cases = str(tmp_path / "cases.txt")
    write_cases(cases)
    p = subprocess.run([build_exe(tmp_path), cases], capture_output=True, text=True)
    assert p.returncode == 77, (p.returncode, p.stdout, p.stderr)
    assert "no CPU fallback" in p.stdout


@pytest.mark.gpu
def test_cpp_filter_mirror_on_gpu(tmp_path):
    # a pure C++ process: the system HIP runtime under /opt/rocm serves it (no torch in this process)
    cases = str(tmp_path / "cases.txt")
    write_cases(cases)
    p = subprocess.run([build_exe(tmp_path), cases], capture_output=True, text=True)
    assert p.returncode == 0, (p.returncode, p.stdout, p.stderr)
    assert "ok" in p.stdout
