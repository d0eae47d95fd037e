"""CPU checks of the covered level's boundary (include/nmi_hip.h: nmi_level_set_coverage, nmi_level_copy_coverage).  No device
needed: every call below is rejected before anything touches a device."""
import ctypes as C

import pytest

from orbslam2_nmi_amd import build as nmi_build
from orbslam2_nmi_amd import capi

COVERED_LEVEL = ("nmi_level_set_coverage", "nmi_level_copy_coverage")


@pytest.fixture(scope="module")
def lib():
    nmi_build.build()
    return capi.load_library()


def test_covered_level_symbols_declared_bound_exported(lib):
    from test_capi_symbols import declared_symbols
    raw = C.CDLL(capi.library_path())
    for name in COVERED_LEVEL:
        assert name in declared_symbols(), name
        assert name in capi.EXPORTED_SYMBOLS, name
        assert hasattr(raw, name), f"libnmi_hip.so does not export {name}"
        assert getattr(lib, name).argtypes, f"{name} has no argtypes"
    assert lib.nmi_abi_version() == 2  # additive: no bump


def test_covered_level_calls_reject_a_null_level(lib):
    fake = C.c_void_p(16)  # never dereferenced: the NULL level is rejected first
    counts = (C.c_int32 * 4)()
    for enabled in (0, 1, 2, -1):
        for mask in (None, fake):
            assert lib.nmi_level_set_coverage(None, enabled, mask) == capi.ERR_INVALID_ARGUMENT
    assert lib.nmi_level_copy_coverage(None, None, None, None) == capi.ERR_INVALID_ARGUMENT
    assert lib.nmi_level_copy_coverage(None, fake, fake, counts) == capi.ERR_INVALID_ARGUMENT


def test_covered_level_argument_checks_come_before_the_level(lib):
    """enabled outside {0, 1} and a mask with enabled = 0 are refused on the arguments alone, before the level is looked at."""
    fake_level, fake_mask = C.c_void_p(16), C.c_void_p(32)
    assert lib.nmi_level_set_coverage(fake_level, 2, None) == capi.ERR_INVALID_ARGUMENT
    assert lib.nmi_level_set_coverage(fake_level, -1, fake_mask) == capi.ERR_INVALID_ARGUMENT
    assert lib.nmi_level_set_coverage(fake_level, 0, fake_mask) == capi.ERR_INVALID_ARGUMENT


def test_python_wrapper_has_the_level_coverage_methods():
    assert callable(getattr(capi.NmiLevel, "set_coverage", None)) and callable(getattr(capi.NmiLevel, "coverage", None))
