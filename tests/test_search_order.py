"""CPU test: the visiting orders of csrc/nmi_search_plan.h -- build_search_order, which keeps one warp per workgroup of a launch so that
nmi_grid_kernel forms the frame marginal once per workgroup -- compiled with plain g++ under ASan / UBSan and checked by
tests/native/search_order.cpp: a permutation for every S, Wn in 1..40 on 1, 8, 64, 243, 248, 256 and 304 workgroups; one warp per workgroup
for 27 x 27 on 243 and 256 and 64 x 64 on 256; at most 14 images per XCD and round there; today's tile order wherever no split exists."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_search_orders_are_permutations_that_keep_a_warp_per_workgroup(tmp_path):
    exe = tmp_path / "search_order"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "orbslam2_nmi_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "search_order.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "search order ok" in r.stdout
