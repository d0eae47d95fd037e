"""CPU checks of the masked / covered stream boundary (include/nmi_hip.h: nmi_pack_mask_bits, nmi_stream_submit_masked[_block],
nmi_stream_submit_covered[_block], nmi_stream_copy_counts): declared, bound, exported, additive (ABI 2), NULL handles
rejected.  No device needed; the GPU tier is tests/test_stream_masked.py."""
import ctypes as C

import pytest

from orbslam2_nmi_amd import build as nmi_build
from orbslam2_nmi_amd import capi

STREAM_MASKED = ("nmi_pack_mask_bits", "nmi_stream_submit_masked", "nmi_stream_submit_masked_block", "nmi_stream_submit_covered",
                 "nmi_stream_submit_covered_block", "nmi_stream_copy_counts")


@pytest.fixture(scope="module")
def lib():
    nmi_build.build()
    return capi.load_library()


def test_stream_masked_symbols_declared_bound_exported(lib):
    from test_capi_symbols import declared_symbols
    raw = C.CDLL(capi.library_path())
    for name in STREAM_MASKED:
        assert name in declared_symbols(), name
        assert name in capi.EXPORTED_SYMBOLS, name
        assert hasattr(raw, name), f"libnmi_hip.so does not export {name}"
        assert getattr(lib, name).argtypes, f"{name} has no argtypes"
    assert lib.nmi_abi_version() == 2  # additive: no bump


def test_stream_masked_entry_points_reject_null(lib):
    t = C.c_int64(0)
    fake = C.c_void_p(16)  # never dereferenced: the NULL stream / context is rejected first
    E = capi.ERR_INVALID_ARGUMENT
    assert lib.nmi_pack_mask_bits(None, fake, 1, fake) == E
    assert lib.nmi_stream_submit_masked(None, fake, 1, None, None, None, 0, C.byref(t)) == E
    assert lib.nmi_stream_submit_masked_block(None, fake, 1, 0, 1, None, None, None, 0, 0, 1, None, C.byref(t)) == E
    assert lib.nmi_stream_submit_covered(None, fake, fake, 1, None, None, None, 0, C.byref(t)) == E
    assert lib.nmi_stream_submit_covered_block(None, fake, fake, 1, 0, 1, None, None, None, 0, 0, 1, None, C.byref(t)) == E
    assert lib.nmi_stream_copy_counts(None, 0, (C.c_int32 * 1)(), 1) == E
