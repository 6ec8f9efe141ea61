"""The plan of the exact scan without a GPU (kektordb_amd/csrc/kdb_flat_plan.h): the host decides from it which ranking kernel runs,
how many stripes, the list capacities, whether a seed launch goes first and where every scratch region lies; the kernels resolve
their stripes and check the seed launch with the same two functions.  A stand-alone C++ program built with AddressSanitizer and
UBSan sweeps the geometry and the plan's invariants (regions in order, aligned, disjoint, as large as every layout that shares
them) and compares fs_plan with the figures it produced while it still lived in flat_scan.hip."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_flat_plan_geometry_invariants_and_literals_under_address_and_ub_sanitizers(tmp_path):
    exe = str(tmp_path / "flat_plan_test")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Werror",
           "-I", os.path.join(ROOT, "kektordb_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "flat_plan_test.cpp"), "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.strip() == "ok" and not r.stderr, (r.stdout, r.stderr[-4000:])
