"""The rules of a mixed search launch without a GPU (kektordb_amd/csrc/kdb_mixed_plan.h): a query's effective ef (the refine boost,
then max(ef, k)), the capacity of a launch from its largest effective ef (the top of the beam class), the predicate the kernels apply
to every query, the admission of a late caller to a running open launch, and the stride of a launch that stays open.  A stand-alone
C++ program built with AddressSanitizer and UBSan checks the figures and the edges."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mixed_plan_rules_under_address_and_ub_sanitizers(tmp_path):
    exe = str(tmp_path / "mixed_plan_test")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Werror",
           "-I", os.path.join(ROOT, "kektordb_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "mixed_plan_test.cpp"), "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.strip() == "ok" and not r.stderr, (r.stdout, r.stderr[-4000:])
