"""SURVEY.md row a14 pinned to the REFERENCE's object code.

tests/golden/search_kernel_ref.npz holds the answers of /root/reference/Thirdparty/Localization/nmiSearchKernel.cpp,
compiled unmodified (oracle/Makefile target _ref, driver oracle/ref_search_kernel_driver.cpp), on 3000 seeded grid
descriptors: isMiddle() (:99-102), counts and steps after each resizeKernel() (:104-141, bit patterns), the operator<<
text (:183-195), and a scripted walk over the constructors, setters and resets (:25-98,143-158).  Checked here, with
equality on every bit and byte: the C entry points nmi_sk_* (include/nmi_host.h) through ctypes, and the C++ class
orbslam2_nmi_amd/host/nmi_search_kernel.hpp by compiling the very same driver source against it."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from orbslam2_nmi_amd import hostapi as H


@pytest.fixture(scope="module")
def ref():
    g = np.load(os.path.join(GOLDEN, "search_kernel_ref.npz"))
    inputs = g["inputs"].tobytes().decode().splitlines()
    outputs = g["outputs"].tobytes().decode("latin-1").split("\n")
    assert len(outputs) == 3 * len(inputs) + 1 and outputs[-1] == ""
    return inputs, outputs, g


def _bits_to_f32(u):
    return np.array([u], np.uint32).view(np.float32)[0]


def test_c_entry_points_equal_reference_object_code(ref):
    inputs, outputs, _ = ref
    lib = H._lib()
    props = H.properties_default()
    buf = C.create_string_buffer(512)
    n_mid = n_collapsed = 0
    for i, line in enumerate(inputs):
        t = line.split()
        num = [int(x) for x in t[0:6]]
        step = [_bits_to_f32(int(x, 16)) for x in t[6:12]]
        best = [int(x) for x in t[12:18]]
        nmi, R = _bits_to_f32(int(t[18], 16)), int(t[19])
        k = H.SearchKernel.make(num, step, best=best, nmi=nmi)
        exp = outputs[3 * i].split()
        lib.nmi_sk_format(C.byref(k), buf, 512)
        assert buf.value.decode("latin-1") == outputs[3 * i + 1], (i, line)
        assert int(exp[0]) == lib.nmi_sk_is_middle(C.byref(k)), (i, line)
        n_mid += int(exp[0])
        for r in range(R + 1):
            e = exp[1 + 12 * r: 13 + 12 * r]
            assert [int(x) for x in e[:6]] == list(k.num), (i, r, line)
            got = np.array(list(k.step), np.float32).view(np.uint32)
            assert [int(x, 16) for x in e[6:]] == [int(x) for x in got], (i, r, line)
            if r < R:
                lib.nmi_sk_resize(C.byref(k), C.byref(props))
        n_collapsed += int(list(k.num) != num)
        assert list(k.best) == best and np.float32(k.nmi).view(np.uint32) == int(t[18], 16)  # resize leaves them alone
        lib.nmi_sk_format(C.byref(k), buf, 512)
        assert buf.value.decode("latin-1") == outputs[3 * i + 2], (i, line)
    assert n_mid > 20 and n_collapsed > 300  # the fixture does exercise both branches


def test_cpp_class_replays_the_reference_driver(ref, tmp_path):
    """The driver source written against the reference's header compiles unchanged against host/nmi_search_kernel.hpp
    (same public names) and prints the same bytes as the reference's object code did."""
    inputs, _, g = ref
    exe = tmp_path / "replay"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off",
                           "-I" + os.path.join(ROOT, "tests", "native", "ref_alias"),
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "orbslam2_nmi_amd", "host"),
                           os.path.join(ROOT, "oracle", "ref_search_kernel_driver.cpp"),
                           os.path.join(ROOT, "orbslam2_nmi_amd", "host", "nmi_driver.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], input=g["inputs"].tobytes(), capture_output=True, check=True, timeout=120).stdout
    assert out == g["outputs"].tobytes()
    walk = subprocess.run([str(exe), "walk"], capture_output=True, check=True, timeout=60).stdout
    assert walk == g["walk"].tobytes()


def test_fixture_is_what_the_reference_build_prints(ref):
    """Where build() made oracle/_ref/ref_search_kernel (the reference's sources were at hand, oracle/Makefile) the committed
    fixture must be reproducible from that binary; without it the fixture stands alone."""
    exe = os.path.join(ROOT, "oracle", "_ref", "ref_search_kernel")
    if not os.access(exe, os.X_OK):
        pytest.skip("oracle/_ref/ref_search_kernel not built (the reference's sources were not available to build())")
    _, _, g = ref
    out = subprocess.run([exe], input=g["inputs"].tobytes(), capture_output=True, check=True, timeout=120).stdout
    assert out == g["outputs"].tobytes()
    assert subprocess.run([exe, "walk"], capture_output=True, check=True).stdout == g["walk"].tobytes()
