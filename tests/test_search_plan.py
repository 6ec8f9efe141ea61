"""The launch plan of hnsw_search_kernel without a GPU (kektordb_amd/csrc/kdb_search_plan.h): the class boundaries of a walk (beam
slots, visited hash, large hash), the LDS bytes of a workgroup against a restatement of the kernel's own LDS carve -- float32 and
int8 keys, three row widths, every beam storage, one, two and four waves per query, hash, large hash and un-mark list, short and
full pending lists --, the ladders of the six beams the GPU parity module walks, and what is left of a ladder at the 160 KiB limit.
A stand-alone C++ program built with AddressSanitizer and UBSan."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_search_plan_matches_the_kernels_lds_carve_under_address_and_ub_sanitizers(tmp_path):
    exe = str(tmp_path / "search_plan_test")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Werror",
           "-I", os.path.join(ROOT, "kektordb_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "search_plan_test.cpp"), "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.strip() == "ok" and not r.stderr, (r.stdout, r.stderr[-4000:])
