"""CPU test: csrc/nmi_search_plan.h -- plan_search, the one function that decides which kernel scores a search -- compiled with
plain g++ under ASan / UBSan (the header depends on nothing from HIP) and checked against the literal policy table of
tests/native/search_plan.cpp: 256 compute units, the boundaries the header's comments name."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plan_search_holds_the_documented_policy_table(tmp_path):
    exe = tmp_path / "search_plan"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "orbslam2_nmi_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "search_plan.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "search plan ok" in r.stdout
