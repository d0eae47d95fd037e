"""CPU checks of the masked search's boundary (include/nmi_hip.h, nmi_warp_stack_masked / nmi_search_grid_masked /
nmi_last_mask_counts) and self-checks of the numpy twin of the warp masks.  No device needed."""
import ctypes as C

import numpy as np
import pytest

from helpers import masked_np as mnp
from orbslam2_nmi_amd import build as nmi_build
from orbslam2_nmi_amd import capi

MASKED = ("nmi_warp_stack_masked", "nmi_search_grid_masked", "nmi_last_mask_counts")


@pytest.fixture(scope="module")
def lib():
    nmi_build.build()
    return capi.load_library()


def test_masked_symbols_declared_bound_exported(lib):
    from test_capi_symbols import declared_symbols
    raw = C.CDLL(capi.library_path())
    for name in MASKED:
        assert name in declared_symbols(), name
        assert name in capi.EXPORTED_SYMBOLS, name
        assert hasattr(raw, name), f"libnmi_hip.so does not export {name}"
        assert getattr(lib, name).argtypes, f"{name} has no argtypes"
    assert lib.nmi_abi_version() == 2  # additive: no bump


def test_masked_entry_points_reject_null(lib):
    i64, f32, i32 = C.c_int64(0), C.c_float(0), (C.c_int32 * 4)()
    fake = C.c_void_p(16)  # never dereferenced: the NULL context is rejected first
    # NULL context
    assert lib.nmi_search_grid_masked(None, fake, 1, fake, fake, 1, None, C.byref(i64), C.byref(f32)) == capi.ERR_INVALID_ARGUMENT
    assert lib.nmi_warp_stack_masked(None, fake, None, (C.c_double * 9)(), 1, fake, fake) == capi.ERR_INVALID_ARGUMENT
    assert lib.nmi_last_mask_counts(None, i32, 1) == capi.ERR_INVALID_ARGUMENT
    # NULL context and NULL mask
    assert lib.nmi_search_grid_masked(None, fake, 1, fake, None, 1, None, C.byref(i64), C.byref(f32)) == capi.ERR_INVALID_ARGUMENT
    assert lib.nmi_warp_stack_masked(None, fake, None, (C.c_double * 9)(), 1, fake, None) == capi.ERR_INVALID_ARGUMENT


def test_twin_identity_is_all_valid():
    m = mnp.warp_masks((48, 64), [np.eye(3)])
    assert m.shape == (1, 48, 64) and m.all()


def test_twin_half_pixel_shift_invalidates_last_column():
    # forward translation by -0.5 px: the source of x is x + 0.5, whose taps are x and x + 1 -- the last column has no x + 1
    M = np.array([[1, 0, -0.5], [0, 1, 0], [0, 0, 1]], np.float64)
    m = mnp.warp_masks((48, 64), [M])[0]
    assert not m[:, -1].any() and m[:, :-1].all()
    # the same along rows
    M = np.array([[1, 0, 0], [0, 1, -0.5], [0, 0, 1]], np.float64)
    m = mnp.warp_masks((48, 64), [M])[0]
    assert not m[-1, :].any() and m[:-1, :].all()


def test_twin_frame_mask_hole_grows_by_tap_footprint():
    fm = np.ones((48, 64), np.uint8)
    fm[20, 30] = 0
    # identity: every pixel reads exactly its own tap -- the hole stays one pixel
    m = mnp.warp_masks((48, 64), [np.eye(3)], fm)[0]
    assert np.array_equal(m, fm)
    # half a pixel in both directions: pixel (x, y) reads x, x + 1 and y, y + 1 -- the hole becomes the 2 x 2 block up-left
    M = np.array([[1, 0, -0.5], [0, 1, -0.5], [0, 0, 1]], np.float64)
    m = mnp.warp_masks((48, 64), [M], fm)[0]
    want = np.ones((48, 64), np.uint8)
    want[19:21, 29:31] = 0
    want[:, -1] = 0
    want[-1, :] = 0
    assert np.array_equal(m, want)


def test_masked_oracle_all_ones_is_the_unmasked_oracle(golden_grid):
    g = golden_grid
    ones = np.ones_like(g["warp_stack"])
    r, i, b = mnp.masked_search(g["render_stack"], g["warp_stack"], ones)
    assert (r.view(np.uint32) == g["ratings_rounded"].view(np.uint32)).all()
    assert i == int(g["best_index_rounded"]) and b == g["best_score_rounded"]
