"""The LDS plan of a walking wave of graph construction without a GPU (kektordb_amd/csrc/kdb_walk_lds.h): the host sizes the launch
from it and build_search_kernel / refine_search_kernel / add_link_kernel take their pointers from it.  A stand-alone C++ program
built with AddressSanitizer and UBSan checks that the regions are in order, aligned, never overlap and end where the host's byte
count ends, and that beam storage, capacities and bytes are the figures the host sites computed by hand before the plan existed."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_walk_plan_layout_under_address_and_ub_sanitizers(tmp_path):
    exe = str(tmp_path / "walk_plan_test")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Werror",
           "-I", os.path.join(ROOT, "kektordb_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "walk_plan_test.cpp"), "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.strip() == "ok" and not r.stderr, (r.stdout, r.stderr[-4000:])
