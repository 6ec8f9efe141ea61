"""MicroBatcher (include/kektor_hip.hpp) and requests that differ in k and efSearch, tests/cpp/mixed_batcher_test.cpp: over an index
that offers SearchMixed the callers of one allow list share a batch whatever they ask for; a test double without it keeps the
(k, efSearch, allow list) keying.  The CPU half runs on test doubles; the GPU half on a real index against SearchWithScores one by one."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "mixed_batcher_test.cpp")


def test_mixed_batcher_keying_on_test_doubles(tmp_path):
    exe = str(tmp_path / "mixed_batcher_test")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), SRC, "-pthread", "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok"), (r.stdout[-2000:], r.stderr[-4000:])


@pytest.mark.gpu
def test_mixed_batcher_on_gpu(tmp_path):
    import kektordb_amd
    kektordb_amd.build_library()
    exe = str(tmp_path / "mixed_batcher_test_gpu")
    libdir = os.path.dirname(kektordb_amd.LIB_PATH)
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-DMIXED_BATCHER_GPU", "-I", os.path.join(ROOT, "include"), SRC, "-L", libdir, "-lkektor_hip",
           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-pthread", "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)   # a pure C++ process (no torch in it)
    assert r.returncode == 0 and "ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
