"""CPU checks of the masked level's boundary (include/nmi_hip.h: nmi_level_set_masks, nmi_level_copy_masks).  No device
needed: every call below is rejected before anything touches a device."""
import ctypes as C

import pytest

from orbslam2_nmi_amd import build as nmi_build
from orbslam2_nmi_amd import capi

MASKED_LEVEL = ("nmi_level_set_masks", "nmi_level_copy_masks")


@pytest.fixture(scope="module")
def lib():
    nmi_build.build()
    return capi.load_library()


def test_masked_level_symbols_declared_bound_exported(lib):
    from test_capi_symbols import declared_symbols
    raw = C.CDLL(capi.library_path())
    for name in MASKED_LEVEL:
        assert name in declared_symbols(), name
        assert name in capi.EXPORTED_SYMBOLS, name
        assert hasattr(raw, name), f"libnmi_hip.so does not export {name}"
        assert getattr(lib, name).argtypes, f"{name} has no argtypes"
    assert lib.nmi_abi_version() == 2  # additive: no bump


def test_masked_level_calls_reject_a_null_level(lib):
    fake = C.c_void_p(16)  # never dereferenced: the NULL level is rejected first
    counts = (C.c_int32 * 4)()
    assert lib.nmi_level_set_masks(None, 1, None) == capi.ERR_INVALID_ARGUMENT
    assert lib.nmi_level_set_masks(None, 1, fake) == capi.ERR_INVALID_ARGUMENT
    assert lib.nmi_level_set_masks(None, 0, None) == capi.ERR_INVALID_ARGUMENT
    assert lib.nmi_level_set_masks(None, 0, fake) == capi.ERR_INVALID_ARGUMENT   # (a mask with enabled = 0, too)
    assert lib.nmi_level_copy_masks(None, None, None) == capi.ERR_INVALID_ARGUMENT
    assert lib.nmi_level_copy_masks(None, fake, counts) == capi.ERR_INVALID_ARGUMENT


def test_python_wrapper_has_the_level_mask_methods():
    assert callable(getattr(capi.NmiLevel, "set_masks", None)) and callable(getattr(capi.NmiLevel, "masks", None))
