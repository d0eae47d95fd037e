"""Covered NMI search on the device (nmi_search_grid_covered, nmi_last_cover_counts): masks on both sides, against
nmi_search_grid_masked and the numpy restatement (tests/helpers/covered_np.py).  Rating tables compared with == on the bits."""
import numpy as np
import pytest
import torch

from helpers import covered_np as cnp
from oracle import binding as oc
from orbslam2_nmi_amd import capi, synthetic as sy

pytestmark = pytest.mark.gpu
SHIFT = {256: 0, 128: 1, 64: 2, 32: 3, 16: 4}


@pytest.fixture(scope="module", autouse=True)
def _device():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    capi.load_library()  # raises if the HIP library is missing: there is no fallback


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def misaligned(a):
    """A contiguous device copy of `a` that starts one byte past a 16-byte boundary."""
    a = np.ascontiguousarray(a)
    buf = torch.empty(a.size + 16, dtype=torch.uint8, device="cuda")
    v = buf[1:1 + a.size].view(*a.shape)
    v.copy_(torch.from_numpy(a.astype(np.uint8)))
    return v


def bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def ctx_for(rs, bins, mode, use_bg, bottom_up, options=None):
    h, w = rs.shape[1:]
    ctx = capi.NmiContext(w, h, bins=bins, mode=mode, use_bg=use_bg, render_bottom_up=bottom_up)
    for k, v in (options or {}).items():
        ctx.set_option(k, v)
    return ctx


def gpu_covered(rs, ws, wm, rm, bins=256, mode=capi.MODE_SUC, use_bg=True, bottom_up=True, options=None, place=dev):
    with ctx_for(rs, bins, mode, use_bg, bottom_up, options) as ctx:
        ratings = torch.full((ws.shape[0], rs.shape[0]), -7.0, dtype=torch.float32, device="cuda")
        idx, best = ctx.search_grid_covered(place(rs), place(rm), place(ws), place(wm), ratings)
        counts = ctx.cover_counts(ws.shape[0] * rs.shape[0]).reshape(ws.shape[0], rs.shape[0])
    return ratings.cpu().numpy(), idx, best, counts


def gpu_masked(rs, ws, wm, bins=256, mode=capi.MODE_SUC, use_bg=True, bottom_up=True, place=dev):
    with ctx_for(rs, bins, mode, use_bg, bottom_up) as ctx:
        ratings = torch.full((ws.shape[0], rs.shape[0]), -7.0, dtype=torch.float32, device="cuda")
        idx, best = ctx.search_grid_masked(place(rs), place(ws), place(wm), ratings)
    return ratings.cpu().numpy(), idx, best


def check_model(rs, ws, wm, rm, bins=256, mode=capi.MODE_SUC, use_bg=True, bottom_up=True, options=None, place=dev):
    got, idx, best, counts = gpu_covered(rs, ws, wm, rm, bins, mode, use_bg, bottom_up, options, place)
    want, wi, wb, wc = cnp.covered_search(rs, ws, wm, rm, SHIFT[bins], use_bg, bottom_up, mode)
    bad = np.argwhere(bits(got) != bits(want))
    assert bad.size == 0, (bad[:5], got[tuple(bad[0])], want[tuple(bad[0])])
    assert (idx, bits(best)) == (wi, bits(wb))
    assert np.array_equal(counts, wc)
    return got, counts


# ---- 1. all-ones render masks == nmi_search_grid_masked -------------------------------------------------------------------
@pytest.mark.parametrize("bins", [256, 64])
@pytest.mark.parametrize("use_bg", [True, False])
@pytest.mark.parametrize("mode", [capi.MODE_SUC, capi.MODE_ENMI])
@pytest.mark.parametrize("bottom_up", [True, False])
def test_all_ones_render_masks_equal_masked_sweep(bins, use_bg, mode, bottom_up):
    wl = sy.workload(64, 48, 8, 9, seed=11, bottom_up=bottom_up)
    rs, ws = wl["render_stack"], wl["warp_stack"]
    wm = (np.random.default_rng(3).random(ws.shape) < 0.85).astype(np.uint8)
    got, idx, best, _ = gpu_covered(rs, ws, wm, np.ones_like(rs), bins, mode, use_bg, bottom_up)
    ref, ri, rb = gpu_masked(rs, ws, wm, bins, mode, use_bg, bottom_up)
    assert (bits(got) == bits(ref)).all() and (idx, bits(best)) == (ri, bits(rb))


@pytest.mark.parametrize("shape,S,Wn", [((640, 480), 27, 27), ((1241, 376), 3, 3), ((200, 150), 4, 5), ((24, 20), 5, 4)],
                         ids=["640x480", "1241x376", "200x150", "24x20"])
@pytest.mark.parametrize("use_bg", [True, False])
def test_all_ones_render_masks_equal_masked_shapes(shape, S, Wn, use_bg):
    w, h = shape
    wl = sy.workload(w, h, S, Wn, seed=7)
    rs, ws = wl["render_stack"], wl["warp_stack"]
    wm = np.ones_like(ws)
    wm[:, : h // 5] = 0
    got, idx, best, counts = gpu_covered(rs, ws, wm, np.ones_like(rs), use_bg=use_bg)
    ref, ri, rb = gpu_masked(rs, ws, wm, use_bg=use_bg)
    assert (bits(got) == bits(ref)).all() and (idx, bits(best)) == (ri, bits(rb))
    assert (counts == w * (h - h // 5)).all()
    # both sides all ones: nmi_search_grid's bits
    with capi.NmiContext(w, h, use_bg=use_bg) as ctx:
        plain = torch.zeros((Wn, S), dtype=torch.float32, device="cuda")
        pi, pb = ctx.search_grid(dev(rs), dev(ws), plain)
    got1, i1, b1, _ = gpu_covered(rs, ws, np.ones_like(ws), np.ones_like(rs), use_bg=use_bg)
    assert (bits(got1) == bits(plain.cpu().numpy())).all() and (i1, bits(b1)) == (pi, bits(pb))


def test_all_ones_render_masks_misaligned_stacks():
    wl = sy.workload(160, 120, 4, 5, seed=9)
    rs, ws = wl["render_stack"], wl["warp_stack"]
    wm = (np.random.default_rng(4).random(ws.shape) < 0.7).astype(np.uint8)
    got, idx, best, _ = gpu_covered(rs, ws, wm, np.ones_like(rs), place=misaligned)
    ref, ri, rb = gpu_masked(rs, ws, wm)
    assert (bits(got) == bits(ref)).all() and (idx, bits(best)) == (ri, bits(rb))


# ---- 2. masks on both sides == the model ------------------------------------------------------------------------------
def structured(rng, n, h, w):
    m = np.ones((n, h, w), np.uint8)
    for k in range(n):
        kind = k % 5
        if kind == 1:
            m[k] = (rng.random((h, w)) < 0.6) * rng.integers(1, 3, (h, w))  # bytes 1 and 2
        elif kind == 2:
            m[k, : h // 2] = 0  # top half only (of the array)
        elif kind == 3:
            y0, x0 = rng.integers(0, h // 2), rng.integers(0, w // 2)
            m[k, y0:y0 + h // 3, x0:x0 + w // 3] = 0
        elif kind == 4:
            m[k] = 2
    return m


@pytest.mark.parametrize("shape,S,Wn,cfg", [
    ((160, 120), 5, 6, dict()),
    ((160, 120), 5, 6, dict(use_bg=False)),
    ((160, 120), 5, 6, dict(bins=64)),
    ((160, 120), 5, 6, dict(bins=64, use_bg=False)),
    ((160, 120), 5, 6, dict(bottom_up=False)),
    ((160, 120), 5, 6, dict(mode=capi.MODE_ENMI)),
    ((200, 150), 3, 4, dict()),
    ((24, 20), 5, 4, dict(use_bg=False)),
    ((640, 480), 4, 3, dict()),
], ids=["bg", "bgoff", "64", "64bgoff", "topdown", "enmi", "200x150", "24x20", "640x480"])
def test_masks_equal_model(shape, S, Wn, cfg):
    w, h = shape
    wl = sy.workload(w, h, S, Wn, seed=S * Wn, bottom_up=cfg.get("bottom_up", True))
    rng = np.random.default_rng(w + S)
    wm, rm = structured(rng, Wn, h, w), structured(rng, S, h, w)
    _, counts = check_model(wl["render_stack"], wl["warp_stack"], wm, rm, **cfg)
    # renders of one warp with different coverage: len differs within a warp's row
    assert (counts.max(axis=1) != counts.min(axis=1)).all()


@pytest.mark.parametrize("bottom_up", [True, False])
def test_top_half_render_masks_follow_the_flip(bottom_up):
    w, h = 64, 48
    wl = sy.workload(w, h, 3, 3, seed=21, bottom_up=bottom_up)
    rm = np.ones((3, h, w), np.uint8)
    rm[:, : h // 2] = 0  # rows 0 .. h/2-1 of the render stack
    wm = np.ones((3, h, w), np.uint8)
    wm[1, h // 2:] = 0
    _, counts = check_model(wl["render_stack"], wl["warp_stack"], wm, rm, bottom_up=bottom_up)
    # with a bottom-up render the uncovered rows are the frame's LOWER half, so warp 1 (lower half masked) keeps all of
    # its pixels; top-down, it keeps none
    assert (counts[1] == (w * h // 2 if bottom_up else 0)).all()


def test_bool_and_misaligned_masks():
    wl = sy.workload(160, 120, 3, 4, seed=5)
    rng = np.random.default_rng(5)
    wm, rm = structured(rng, 4, 120, 160), structured(rng, 3, 120, 160)
    a, ia, ba, ca = gpu_covered(wl["render_stack"], wl["warp_stack"], wm, rm)
    b, ib, bb, cb = gpu_covered(wl["render_stack"], wl["warp_stack"], wm, rm, place=misaligned)
    assert (bits(a) == bits(b)).all() and (ia, bits(ba)) == (ib, bits(bb)) and (ca == cb).all()
    with capi.NmiContext(160, 120) as ctx:
        r = torch.zeros((4, 3), dtype=torch.float32, device="cuda")
        ic, bc = ctx.search_grid_covered(dev(wl["render_stack"]), dev(rm != 0), dev(wl["warp_stack"]), dev(wm != 0), r)
    assert (bits(r.cpu().numpy()) == bits(a)).all() and (ic, bits(bc)) == (ia, bits(ba))


# ---- 3. pixels under a zero mask do not matter; 4. empty intersections score 0 ------------------------------------------
def test_masked_out_pixels_do_not_matter():
    wl = sy.workload(160, 120, 5, 5, seed=4)
    rs, ws = wl["render_stack"], wl["warp_stack"]
    rng = np.random.default_rng(8)
    wm, rm = structured(rng, 5, 120, 160), structured(rng, 5, 120, 160)
    a, ia, ba, _ = gpu_covered(rs, ws, wm, rm)
    ws2 = np.where(wm != 0, ws, rng.integers(0, 256, ws.shape, dtype=np.uint8))
    rs2 = np.where(rm != 0, rs, rng.integers(0, 256, rs.shape, dtype=np.uint8))
    assert (ws2 != ws).any() and (rs2 != rs).any()
    b, ib, bb, _ = gpu_covered(rs2, ws2, wm, rm)
    assert (bits(a) == bits(b)).all() and (ia, bits(ba)) == (ib, bits(bb))


def test_empty_intersection_scores_zero():
    w, h = 64, 48
    wl = sy.workload(w, h, 3, 3, seed=2)
    wm = np.ones((3, h, w), np.uint8)
    wm[0, : h // 2] = 0
    rm = np.ones((3, h, w), np.uint8)
    rm[1, : h // 2] = 0  # bottom-up: the frame's lower half ... 
    rm[2] = 0
    got, counts = check_model(wl["render_stack"], wl["warp_stack"], wm, rm)
    assert (got[:, 2] == 0.0).all() and (counts[:, 2] == 0).all()
    assert counts[0, 1] == 0 and got[0, 1] == 0.0  # ... meets warp 0's upper-half mask: nothing in common


# ---- 5. counter wraps under masks ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [dict(), dict(use_bg=False), dict(bins=64)], ids=["bg", "bgoff", "64bins"])
def test_wrap_under_masks_is_exact(cfg):
    w, h = 640, 480
    rng = np.random.default_rng(2)
    rs = np.full((2, h, w), 200, np.uint8)
    ws = np.full((3, h, w), 100, np.uint8)
    rs[1, :40] = rng.integers(1, 256, (40, w), dtype=np.uint8)
    ws[:, 400:] = rng.integers(1, 256, (80, w), dtype=np.uint8)
    wm = np.ones((3, h, w), np.uint8)
    wm[1, :, :100] = 0
    wm[2] = rng.random((h, w)) < 0.9
    rm = np.ones((2, h, w), np.uint8)
    rm[1, :, 500:] = 0
    mask = cnp.pair_mask(wm[1], rm[0]).astype(np.uint8)
    from helpers import masked_np as mnp
    j, _, _ = mnp.masked_hist(rs[0], ws[1], mask)
    assert j.max() > 65535  # the flat bin wraps a 16-bit counter
    check_model(rs, ws, wm, rm, **cfg)


# ---- 6. the unmasked search's kernel choices do not apply ---------------------------------------------------------------
def test_split_and_content_options_do_not_change_covered_results():
    wl = sy.workload(160, 120, 3, 3, seed=6)
    rng = np.random.default_rng(6)
    wm, rm = structured(rng, 3, 120, 160), structured(rng, 3, 120, 160)
    base, bi, bb, _ = gpu_covered(wl["render_stack"], wl["warp_stack"], wm, rm)
    N = capi.NmiContext
    for opts in ({N.OPT_SPLIT: 8}, {N.OPT_SPLIT: 1, N.OPT_SPLIT_PIXELS: 4}, {N.OPT_SPLIT: 0}, {N.OPT_CONTENT_PATH: 1},
                 {N.OPT_CONTENT_PATH: 0}, {N.OPT_SPLIT: 4, N.OPT_SPLIT_PIXELS: 2, N.OPT_CONTENT_PATH: 1}):
        got, gi, gb, _ = gpu_covered(wl["render_stack"], wl["warp_stack"], wm, rm, options=opts)
        assert (bits(got) == bits(base)).all() and (gi, bits(gb)) == (bi, bits(bb)), opts


def test_null_masks_and_counts_bounds_are_rejected():
    wl = sy.workload(64, 48, 2, 2, seed=1)
    rs, ws = dev(wl["render_stack"]), dev(wl["warp_stack"])
    m = torch.ones_like(ws)
    import ctypes as C
    with capi.NmiContext(64, 48) as ctx:
        lib = capi.load_library()
        i64, f32 = C.c_int64(0), C.c_float(0)
        for rmp, wmp in ((None, m.data_ptr()), (m.data_ptr(), None)):
            assert lib.nmi_search_grid_covered(ctx._h, rs.data_ptr(), rmp, 2, ws.data_ptr(), wmp, 2, None, C.byref(i64),
                                               C.byref(f32)) == capi.ERR_INVALID_ARGUMENT
        assert lib.nmi_search_grid_covered(ctx._h, rs.data_ptr(), m.data_ptr(), 0, ws.data_ptr(), m.data_ptr(), 2, None, C.byref(i64),
                                           C.byref(f32)) == capi.ERR_INVALID_ARGUMENT
        ctx.search_grid_covered(rs, m, ws, m)
        assert (ctx.cover_counts(4) == 64 * 48).all()
        with pytest.raises(Exception):
            ctx.cover_counts(5)
