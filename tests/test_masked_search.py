"""Masked NMI search on the device (nmi_search_grid_masked, nmi_warp_stack_masked, nmi_last_mask_counts) against the numpy
restatement (tests/helpers/masked_np.py): rating tables compared with == on the bits, under the oracle's rounded terms."""
import numpy as np
import pytest
import torch

from helpers import masked_np as mnp
from oracle import binding as oc
from orbslam2_nmi_amd import capi, synthetic as sy

pytestmark = pytest.mark.gpu


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


def gpu_masked(rs, ws, ms, bins=256, mode=capi.MODE_SUC, use_bg=True, bottom_up=True, options=None, place=dev):
    h, w = rs.shape[1:]
    with capi.NmiContext(w, h, bins=bins, mode=mode, use_bg=use_bg, render_bottom_up=bottom_up) as ctx:
        for k, v in (options or {}).items():
            ctx.set_option(k, v)
        ratings = torch.full((ws.shape[0], rs.shape[0]), -7.0, dtype=torch.float32, device="cuda")
        idx, best = ctx.search_grid_masked(place(rs), place(ws), place(ms) if isinstance(ms, np.ndarray) else ms, ratings)
        counts = ctx.mask_counts(ws.shape[0])
    return ratings.cpu().numpy(), idx, best, counts


def gpu_plain(rs, ws, bins=256, mode=capi.MODE_SUC, use_bg=True, bottom_up=True, place=dev):
    h, w = rs.shape[1:]
    with capi.NmiContext(w, h, bins=bins, mode=mode, use_bg=use_bg, render_bottom_up=bottom_up) as ctx:
        ratings = torch.zeros((ws.shape[0], rs.shape[0]), dtype=torch.float32, device="cuda")
        idx, best = ctx.search_grid(place(rs), place(ws), ratings)
    return ratings.cpu().numpy(), idx, best


def check_oracle(rs, ws, ms, bins=256, mode=capi.MODE_SUC, use_bg=True, bottom_up=True, options=None, place=dev):
    got, idx, best, counts = gpu_masked(rs, ws, ms, bins, mode, use_bg, bottom_up, options, place)
    shift = {256: 0, 128: 1, 64: 2, 32: 3, 16: 4}[bins]
    want, wi, wb = mnp.masked_search(rs, ws, ms, shift, use_bg, bottom_up, mode)
    bad = np.argwhere(bits(got) != bits(want))
    assert bad.size == 0, (bad[:5], got[tuple(bad[0])], want[tuple(bad[0])])
    assert (idx, bits(best)) == (wi, bits(wb))
    assert np.array_equal(counts, np.count_nonzero(ms.reshape(ms.shape[0], -1), axis=1))
    libm, _, _ = mnp.masked_search(rs, ws, ms, shift, use_bg, bottom_up, mode, rounded=False)
    assert float(np.abs(got - libm).max()) <= 1e-5
    return got


# ---- 1. all-ones masks == nmi_search_grid ------------------------------------------------------------------------------
def test_all_ones_golden(golden_grid):
    g = golden_grid
    rs, ws = g["render_stack"], g["warp_stack"]
    got, idx, best, _ = gpu_masked(rs, ws, np.ones_like(ws))
    assert (bits(got) == bits(g["ratings_rounded"])).all()
    assert idx == int(g["best_index_rounded"]) and best == g["best_score_rounded"]


@pytest.mark.parametrize("bins", [256, 64])
@pytest.mark.parametrize("use_bg", [True, False])
@pytest.mark.parametrize("mode", [capi.MODE_SUC, capi.MODE_ENMI])
@pytest.mark.parametrize("bottom_up", [True, False])
def test_all_ones_equals_unmasked_sweep(bins, use_bg, mode, bottom_up):
    wl = sy.workload(64, 48, 8, 9, seed=11, bottom_up=bottom_up)
    rs, ws = wl["render_stack"], wl["warp_stack"]
    got, idx, best, _ = gpu_masked(rs, ws, np.ones_like(ws), bins, mode, use_bg, bottom_up)
    ref, ri, rb = gpu_plain(rs, ws, bins, mode, use_bg, bottom_up)
    assert (bits(got) == bits(ref)).all() and (idx, bits(best)) == (ri, bits(rb))


@pytest.mark.parametrize("shape,S,Wn", [((640, 480), 27, 27), ((1241, 376), 3, 3), ((200, 150), 4, 5), ((24, 20), 5, 4)],
                         ids=["729@640x480", "kitti_ragged", "ragged_200", "narrow_24"])
@pytest.mark.parametrize("use_bg", [True, False])
def test_all_ones_equals_unmasked_shapes(shape, S, Wn, use_bg):
    w, h = shape
    wl = sy.workload(w, h, S, Wn, seed=5)
    rs, ws = wl["render_stack"], wl["warp_stack"]
    got, idx, best, _ = gpu_masked(rs, ws, np.ones_like(ws), use_bg=use_bg)
    ref, ri, rb = gpu_plain(rs, ws, use_bg=use_bg)
    assert (bits(got) == bits(ref)).all() and (idx, bits(best)) == (ri, bits(rb))


def test_all_ones_misaligned_stacks():
    wl = sy.workload(160, 120, 4, 6, seed=9)
    rs, ws = wl["render_stack"], wl["warp_stack"]
    got, idx, best, _ = gpu_masked(rs, ws, np.ones_like(ws), place=misaligned)
    ref, ri, rb = gpu_plain(rs, ws)
    assert (bits(got) == bits(ref)).all() and (idx, bits(best)) == (ri, bits(rb))


# ---- 2. random and structured masks == the oracle -------------------------------------------------------------------------
def structured_masks(rng, Wn, h, w):
    ms = np.zeros((Wn, h, w), np.uint8)
    dens = (0.05, 0.5, 0.95)
    for k in range(Wn):
        kind = k % 5
        if kind < 3:
            ms[k] = rng.random((h, w)) < dens[kind]
        elif kind == 3:  # rectangular occluders on an all-valid mask
            ms[k] = 1
            for _ in range(3):
                y0, x0 = rng.integers(0, h), rng.integers(0, w)
                ms[k, y0:y0 + rng.integers(1, h // 2 + 2), x0:x0 + rng.integers(1, w // 2 + 2)] = 0
        else:  # bool-like and 255-valued masks alike: nonzero = valid
            ms[k] = np.where(rng.random((h, w)) < 0.7, 255, 0)
    if Wn >= 2:
        ms[0] = 0                 # an empty warp: its row is all 0.0
        ms[1] = 0
        ms[1, h // 2, w // 3] = 1  # a single valid pixel
    return ms


@pytest.mark.parametrize("shape,S,Wn,cfg", [
    ((160, 120), 1, 1, dict()),
    ((160, 120), 3, 3, dict(use_bg=False)),
    ((160, 120), 9, 9, dict(bins=64, bottom_up=False)),
    ((160, 120), 9, 9, dict(bins=64, use_bg=False, mode=capi.MODE_ENMI)),
    ((640, 480), 27, 27, dict()),
    ((64, 48), 64, 64, dict(use_bg=False)),
    ((1241, 376), 2, 3, dict(use_bg=False, bins=128)),
    ((24, 20), 6, 5, dict(mode=capi.MODE_ENMI)),
], ids=["1", "9_bgoff", "81_64bins_topdown", "81_64bins_bgoff_enmi", "729_640x480", "4096_bgoff", "kitti_ragged", "narrow"])
def test_masks_equal_oracle(shape, S, Wn, cfg):
    w, h = shape
    wl = sy.workload(w, h, S, Wn, seed=S * 31 + Wn, bottom_up=cfg.get("bottom_up", True))
    ms = structured_masks(np.random.default_rng(S + 7 * Wn), Wn, h, w)
    if Wn == 1:
        ms[0] = np.random.default_rng(3).random((h, w)) < 0.5
    got = check_oracle(wl["render_stack"], wl["warp_stack"], ms, **cfg)
    if Wn >= 2:
        assert (got[0] == 0.0).all()


def test_masks_equal_oracle_bool_and_misaligned():
    wl = sy.workload(160, 120, 4, 5, seed=21)
    ms = structured_masks(np.random.default_rng(1), 5, 120, 160)
    # bool tensor: the same bytes
    got, idx, best, counts = gpu_masked(wl["render_stack"], wl["warp_stack"], dev(ms != 0))
    want, wi, wb = mnp.masked_search(wl["render_stack"], wl["warp_stack"], ms)
    assert (bits(got) == bits(want)).all() and (idx, bits(best)) == (wi, bits(wb))
    check_oracle(wl["render_stack"], wl["warp_stack"], ms, place=misaligned)


# ---- 3. invariance -------------------------------------------------------------------------------------------------------
def test_masked_out_pixels_do_not_matter():
    wl = sy.workload(160, 120, 9, 9, seed=4)
    rs, ws = wl["render_stack"], wl["warp_stack"]
    rng = np.random.default_rng(8)
    ms = structured_masks(rng, 9, 120, 160)
    a, ia, ba, _ = gpu_masked(rs, ws, ms)
    ws2 = np.where(ms != 0, ws, rng.integers(0, 256, ws.shape, dtype=np.uint8))
    assert (ws2 != ws).any()
    b, ib, bb, _ = gpu_masked(rs, ws2, ms)
    assert (bits(a) == bits(b)).all() and (ia, bits(ba)) == (ib, bits(bb))


# ---- 4. counter wraps under a mask ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [dict(), dict(use_bg=False), dict(bins=64)], ids=["bg", "bgoff", "64bins"])
def test_wrap_under_mask_is_exact(cfg):
    w, h = 640, 480
    rng = np.random.default_rng(2)
    rs = np.full((2, h, w), 200, np.uint8)
    ws = np.full((3, h, w), 100, np.uint8)
    rs[1, :40] = rng.integers(1, 256, (40, w), dtype=np.uint8)  # some texture
    ws[:, 400:] = rng.integers(1, 256, (80, w), dtype=np.uint8)
    ms = np.ones((3, h, w), np.uint8)
    ms[1, :, :100] = 0
    ms[2] = rng.random((h, w)) < 0.9
    j, _, _ = mnp.masked_hist(rs[0], ws[1], ms[1])
    assert j.max() > 65535  # the flat bin wraps a 16-bit counter
    check_oracle(rs, ws, ms, **cfg)


# ---- 5. counts -----------------------------------------------------------------------------------------------------------
def test_mask_counts():
    wl = sy.workload(64, 48, 2, 6, seed=2)
    ms = structured_masks(np.random.default_rng(5), 6, 48, 64)
    _, _, _, counts = gpu_masked(wl["render_stack"], wl["warp_stack"], ms)
    assert np.array_equal(counts, ms.reshape(6, -1).astype(bool).sum(axis=1))


def test_null_mask_is_rejected():
    with capi.NmiContext(64, 48) as ctx:
        rs = torch.zeros((1, 48, 64), dtype=torch.uint8, device="cuda")
        idx, sc = capi.C.c_int64(0), capi.C.c_float(0)
        rc = ctx._lib.nmi_search_grid_masked(ctx._h, rs.data_ptr(), 1, rs.data_ptr(), None, 1, None, capi.C.byref(idx), capi.C.byref(sc))
        assert rc == capi.ERR_INVALID_ARGUMENT


# ---- 6. producer ---------------------------------------------------------------------------------------------------------
KITTI_K = np.array([[718.856, 0, 607.1928], [0, 718.856, 185.2157], [0, 0, 1]])


@pytest.mark.parametrize("shape", [(1241, 376), (640, 480)])
@pytest.mark.parametrize("with_frame_mask", [False, True])
def test_producer(shape, with_frame_mask):
    w, h = shape
    K = KITTI_K * np.array([[w / 1241], [h / 376], [1]])
    Ms = capi.warp_homographies(K, (3, 3, 3), (0.02, 0.02, 0.05))
    frame = sy.camera_frame(sy.scene(w, h, 17), 18)
    fm = None
    if with_frame_mask:
        fm = np.ones((h, w), np.uint8)
        fm[h // 3:h // 2, w // 4:w // 2] = 0  # e.g. a windshield mount
        fm[np.random.default_rng(1).random((h, w)) < 0.01] = 0
    with capi.NmiContext(w, h) as ctx:
        plain = ctx.warp_stack(dev(frame), Ms).cpu().numpy()
        warps, masks = ctx.warp_stack_masked(dev(frame), Ms, None if fm is None else dev(fm))
        warps, masks = warps.cpu().numpy(), masks.cpu().numpy()
        _, bmasks = ctx.warp_stack_masked(dev(frame), Ms, None if fm is None else dev(fm != 0),
                                          out_masks=torch.empty((27, h, w), dtype=torch.bool, device="cuda"))
    assert np.array_equal(warps, plain)
    want = mnp.warp_masks((h, w), Ms, fm)
    assert np.array_equal(masks, want), np.argwhere(masks != want)[:5]
    assert np.array_equal(bmasks.cpu().numpy(), want != 0)
    assert masks[13].mean() > 0.9  # centre cell: the identity up to the rounding of K R K^-1 (exact identity: test below)
    assert masks.sum() < masks.size  # the rotations have borders


def test_producer_identity():
    w, h = 200, 150
    frame = sy.camera_frame(sy.scene(w, h, 3), 4)
    with capi.NmiContext(w, h) as ctx:
        warps, masks = ctx.warp_stack_masked(dev(frame), np.eye(3)[None])
    assert masks.cpu().numpy().all() and np.array_equal(warps.cpu().numpy()[0], frame)


# ---- 7. end to end -------------------------------------------------------------------------------------------------------
def test_end_to_end_occluder():
    w, h, S, Wn = 160, 120, 27, 27
    wl = sy.workload(w, h, S, Wn, seed=1234)
    frame = wl["frame"].copy()
    frame[30:70, 20:60] = 255  # an occluder pasted into the camera frame ...
    fm = np.ones((h, w), np.uint8)
    fm[30:70, 20:60] = 0  # ... and excluded by the frame mask
    Ms = sy.warp_homographies(sy.intrinsics(w, h), wl["w_counts"], (0.02, 0.02, 0.05))
    with capi.NmiContext(w, h) as ctx:
        warps, masks = ctx.warp_stack_masked(dev(frame), Ms, dev(fm))
        ratings = torch.zeros((Wn, S), dtype=torch.float32, device="cuda")
        idx, best = ctx.search_grid_masked(dev(wl["render_stack"]), warps, masks, ratings)
        warps, masks = warps.cpu().numpy(), masks.cpu().numpy()
    assert idx == wl["planted"], (idx, wl["planted"])
    want, wi, wb = mnp.masked_search(wl["render_stack"], warps, masks)
    assert (bits(ratings.cpu().numpy()) == bits(want)).all() and (idx, bits(best)) == (wi, bits(wb))


# ---- 8. the unmasked search's kernel choices do not apply ------------------------------------------------------------------
def test_split_and_content_options_do_not_change_masked_results():
    wl = sy.workload(160, 120, 3, 3, seed=6)
    ms = structured_masks(np.random.default_rng(6), 3, 120, 160)
    base, bi, bb, _ = gpu_masked(wl["render_stack"], wl["warp_stack"], ms)
    N = capi.NmiContext
    for opts in ({N.OPT_SPLIT: 8}, {N.OPT_SPLIT: 1, N.OPT_SPLIT_PIXELS: 4}, {N.OPT_SPLIT: 0}, {N.OPT_CONTENT_PATH: 1},
                 {N.OPT_CONTENT_PATH: 0}, {N.OPT_SPLIT: 4, N.OPT_SPLIT_PIXELS: 2, N.OPT_CONTENT_PATH: 1}):
        got, gi, gb, _ = gpu_masked(wl["render_stack"], wl["warp_stack"], ms, options=opts)
        assert (bits(got) == bits(base)).all() and (gi, bits(gb)) == (bi, bits(bb)), opts
