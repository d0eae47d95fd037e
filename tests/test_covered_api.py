"""CPU checks of the covered search's boundary (include/nmi_hip.h: nmi_search_grid_covered, nmi_last_cover_counts,
nmi_render_points_masked, nmi_render_mesh_masked) and self-checks of its numpy model.  No device needed."""
import ctypes as C

import numpy as np
import pytest

from helpers import covered_np as cnp
from helpers import masked_np as mnp
from oracle import binding as oc
from orbslam2_nmi_amd import build as nmi_build
from orbslam2_nmi_amd import capi, synthetic as sy

COVERED = ("nmi_render_points_masked", "nmi_render_mesh_masked", "nmi_search_grid_covered", "nmi_last_cover_counts")


@pytest.fixture(scope="module")
def lib():
    nmi_build.build()
    return capi.load_library()


def test_covered_symbols_declared_bound_exported(lib):
    from test_capi_symbols import declared_symbols
    raw = C.CDLL(capi.library_path())
    for name in COVERED:
        assert name in declared_symbols(), name
        assert name in capi.EXPORTED_SYMBOLS, name
        assert hasattr(raw, name), f"libnmi_hip.so does not export {name}"
        assert getattr(lib, name).argtypes, f"{name} has no argtypes"
    assert lib.nmi_abi_version() == 2  # additive: no bump


def test_covered_entry_points_reject_null(lib):
    i64, f32, i32 = C.c_int64(0), C.c_float(0), (C.c_int32 * 4)()
    fake = C.c_void_p(16)  # never dereferenced: the NULL context / mask is rejected first
    mvp = (C.c_float * 16)()
    E = capi.ERR_INVALID_ARGUMENT
    # NULL context
    assert lib.nmi_search_grid_covered(None, fake, fake, 1, fake, fake, 1, None, C.byref(i64), C.byref(f32)) == E
    assert lib.nmi_last_cover_counts(None, i32, 1) == E
    assert lib.nmi_render_points_masked(None, fake, fake, 1, mvp, 1, 1.0, fake, fake) == E
    assert lib.nmi_render_mesh_masked(None, fake, fake, 1, fake, mvp, 1, fake, fake) == E
    # NULL masks (with a NULL context too: either is enough)
    assert lib.nmi_search_grid_covered(None, fake, None, 1, fake, fake, 1, None, C.byref(i64), C.byref(f32)) == E
    assert lib.nmi_search_grid_covered(None, fake, fake, 1, fake, None, 1, None, C.byref(i64), C.byref(f32)) == E
    assert lib.nmi_render_points_masked(None, fake, fake, 1, mvp, 1, 1.0, fake, None) == E
    assert lib.nmi_render_mesh_masked(None, fake, fake, 1, fake, mvp, 1, fake, None) == E


def test_model_all_ones_render_masks_is_the_masked_model():
    wl = sy.workload(40, 30, 3, 4, seed=3)
    rs, ws = wl["render_stack"], wl["warp_stack"]
    rng = np.random.default_rng(1)
    wm = (rng.random(ws.shape) < 0.8).astype(np.uint8)
    got, gi, gb, counts = cnp.covered_search(rs, ws, wm, np.ones_like(rs))
    want, wi, wb = mnp.masked_search(rs, ws, wm)
    assert (got.view(np.uint32) == want.view(np.uint32)).all() and (gi, gb) == (wi, wb)
    assert (counts == np.count_nonzero(wm.reshape(4, -1), axis=1)[:, None]).all()


def test_model_len_is_per_candidate():
    """Two renders with different coverage against one warp: different len, so a per-warp len would be wrong."""
    wl = sy.workload(40, 30, 2, 1, seed=5)
    rs, ws = wl["render_stack"], wl["warp_stack"]
    rm = np.ones_like(rs)
    rm[1, :10] = 0
    wm = np.ones_like(ws)
    r, _, _, counts = cnp.covered_search(rs, ws, wm, rm)
    assert counts[0, 0] == 40 * 30 and counts[0, 1] == 40 * 20
    # the second candidate is NOT the masked search of its pixels with the warp's len
    mask = cnp.pair_mask(wm[0], rm[1]).astype(np.uint8)
    with oc.rounded():
        j, h1, h2 = mnp.masked_hist(rs[1], ws[0], mask)
        per_warp = oc.score_from_hist(j, h1, h2, 40 * 30, oc.MODE_SUC)[0]
    assert r[0, 1] != per_warp


def test_model_flip_and_nonzero_bytes():
    rm = np.zeros((1, 4, 6), np.uint8)
    rm[0, :2] = 2  # the first two rows of a bottom-up render are the frame's last two
    wm = np.ones((1, 4, 6), np.uint8)
    c_up = cnp.cover_counts(wm, rm, True)
    assert c_up[0, 0] == 12 and cnp.pair_mask(wm[0], rm[0], True)[2:].all() and not cnp.pair_mask(wm[0], rm[0], True)[:2].any()
    assert cnp.pair_mask(wm[0], rm[0], False)[:2].all()
    # bytes 1 and 2 both count: no raw AND
    assert cnp.cover_counts(np.ones((1, 4, 6), np.uint8), np.full((1, 4, 6), 2, np.uint8))[0, 0] == 24


def test_twin_single_point_of_size_3_covers_3x3():
    rp = capi.RenderParams(fx=50.0, fy=50.0, cx=32.0, cy=24.0, near_plane=1.0, far_plane=30.0, point_size=3.0)
    m = capi.render_mvp(rp, (0, 0, 0), (0, 0, 1), (0, -1, 0), (0, 0, 0))
    cov = cnp.coverage_twin_points(np.array([[0, 0, 10.0]], np.float32), m[None], 64, 48, 3.0)
    assert cov.shape == (1, 48, 64) and cov.sum() == 9
    ys, xs = np.nonzero(cov[0])
    assert xs.max() - xs.min() == 2 and ys.max() - ys.min() == 2
