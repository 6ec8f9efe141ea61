"""The plan of the heap-order walk without a GPU (kektordb_amd/csrc/kdb_heap_plan.h): the visited hash, the result heap's place, the
candidate heap's capacity and its LDS part, and the LDS bytes of a workgroup -- for every ef from 1 to 2000, float32 and int8 keys,
four row widths and three index sizes -- against the bounds every plan keeps and against a restatement of heap_walk_kernel's own LDS
carve.  A stand-alone C++ program built with AddressSanitizer and UBSan."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_heap_plan_matches_the_kernels_lds_carve_under_address_and_ub_sanitizers(tmp_path):
    exe = str(tmp_path / "heap_plan_test")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Werror",
           "-I", os.path.join(ROOT, "kektordb_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "heap_plan_test.cpp"), "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.strip() == "ok" and not r.stderr, (r.stdout, r.stderr[-4000:])
