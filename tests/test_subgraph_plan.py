"""The plan of the subgraph kernels without a GPU (kdb_subgraph_plan.h): a stand-alone C++ program built with ASan and UBSan."""
import os
import subprocess


def test_subgraph_plan_under_address_and_ub_sanitizers(tmp_path):
    ROOT, exe = os.path.dirname(os.path.dirname(os.path.abspath(__file__))), str(tmp_path / "subgraph_plan_test")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Werror",
           "-I", os.path.join(ROOT, "kektordb_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "subgraph_plan_test.cpp"), "-o", exe]
    subprocess.run(cmd, check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert (r.returncode, r.stdout.strip(), r.stderr) == (0, "ok", ""), (r.stdout[-2000:], r.stderr[-4000:])
