"""CPU test: csrc/nmi_mem.h -- the owners of device memory (buffers, pinned buffers, events, streams, the upload ring) and their
one grow rule -- compiled with plain g++ under ASan / UBSan against the HIP runtime that tests/native/device_memory.cpp defines
itself (malloc / free behind every allocation, a call log, a switch that fails the Nth call): the order of wait, free and
allocate, what a failure leaves behind, and no leak or second release for a failure at every call of a scripted scenario."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_owners_release_once_and_grow_by_one_rule(tmp_path):
    exe = tmp_path / "device_memory"
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"),
                           "-I" + os.path.join(ROOT, "orbslam2_nmi_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "device_memory.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "device memory ok" in r.stdout
