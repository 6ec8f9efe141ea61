"""Index::GetVectors / Index::SearchSimilar of the C++ host mirror (include/kektor_hip.hpp): tests/cpp/by_id_test.cpp compiles with
plain g++ against the header and links the shared library; without a GPU it fails loudly (exit 77), on the GPU GetVectors followed
by SearchWithScores equals SearchSimilar for 50 ids of a 2000 x 16 L2 index, self ranks first and is absent with dropSelf."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_exe(tmp_path):
    import kektordb_amd
    kektordb_amd.build_library()
    exe = str(tmp_path / "by_id_test")
    libdir = os.path.dirname(kektordb_amd.LIB_PATH)
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "by_id_test.cpp"), "-L", libdir, "-lkektor_hip",
           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-pthread", "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    return exe


@pytest.mark.skipif(__import__("conftest").HAS_GPU, reason="CPU-only behaviour")
def test_cpp_by_id_links_and_fails_loudly_without_gpu(tmp_path):
    p = subprocess.run([build_exe(tmp_path)], capture_output=True, text=True)
    assert p.returncode == 77, (p.returncode, p.stdout, p.stderr)
    assert "no CPU fallback" in p.stdout


@pytest.mark.gpu
def test_cpp_by_id_on_gpu(tmp_path):
    # a pure C++ process: the system HIP runtime under /opt/rocm serves it (no torch in this process)
    p = subprocess.run([build_exe(tmp_path)], capture_output=True, text=True)
    assert p.returncode == 0, (p.returncode, p.stdout, p.stderr)
    assert "ok" in p.stdout
