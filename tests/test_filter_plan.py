"""The plan of filter_eval_kernel without a GPU (kektordb_amd/csrc/kdb_filter_plan.h): tiles that cover every word of a list exactly
once, program chunks that cover every program exactly once, term validation, the 64-bit exact layout of the staged programs, and the
value of a program (kdb_filter_run, the function the kernel calls).  A stand-alone C++ program built with AddressSanitizer and UBSan
checks them."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_filter_plan_under_address_and_ub_sanitizers(tmp_path):
    exe = str(tmp_path / "filter_plan_test")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Werror",
           "-I", os.path.join(ROOT, "kektordb_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "filter_plan_test.cpp"), "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.strip() == "ok" and not r.stderr, (r.stdout, r.stderr[-4000:])
