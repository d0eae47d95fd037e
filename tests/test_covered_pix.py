"""GPU tests (-m gpu) of the covered pixel-range kernel (csrc/nmi_covered_pix_kernel.hip): nmi_search_grid_covered on mid-size
grids, against NMI_OPT_SPLIT 0 (the covered grid kernel) and the covered numpy model (tests/helpers/covered_np.py, oracle terms
rounded).  Rating tables compared with == on the bits."""
import time

import numpy as np
import pytest

from helpers import covered_np as cnp
from helpers import masked_np as mnp
from helpers import pix_ranges_np as prn
from orbslam2_nmi_amd import capi, synthetic as sy

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _device():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    capi.load_library()  # raises if the HIP library is missing: there is no fallback


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def covered(rs, ws, wm, rm, bottom_up=True, options=None, use_bg=True):
    """-> (ratings, index, score, counts, pix_status + pix_heal_counts, compute units) of one nmi_search_grid_covered on a fresh context."""
    S, Wn = rs.shape[0], ws.shape[0]
    h, w = rs.shape[1:]
    with capi.NmiContext(w, h, render_bottom_up=bottom_up, use_bg=use_bg) as ctx:
        for k, v in (options or {}).items():
            ctx.set_option(k, v)
        t = torch.full((Wn, S), -3.0, device="cuda")
        idx, best = ctx.search_grid_covered(dev(rs), dev(rm), dev(ws), dev(wm), t)
        counts = ctx.cover_counts(S * Wn).reshape(Wn, S)
        st = {**ctx.pix_status(), **ctx.pix_heal_counts()}
        cus = ctx.info()["compute_units"]
    return t.cpu().numpy(), idx, best, counts, st, cus


def masks_for(S, Wn, w, h, seed):
    rng = np.random.default_rng(seed)
    wm = (rng.random((Wn, h, w)) < 0.8).astype(np.uint8)
    wm[:, h - h // 5:] = 0
    rm = np.ones((S, h, w), np.uint8)
    for s in range(S):
        y0, x0 = rng.integers(0, h // 2), rng.integers(0, w // 2)
        rm[s, y0:y0 + h // 3, x0:x0 + w // 3] = 0      # a hole in the map's coverage
        if s % 3 == 1:
            rm[s] *= rng.integers(1, 3, (h, w)).astype(np.uint8)  # bytes 1 and 2 both mean "covered"
    return wm, rm


@pytest.mark.parametrize("S,Wn,w,h", [(9, 9, 160, 128), (11, 3, 160, 128), (1, 128, 160, 128), (85, 1, 176, 96), (16, 8, 160, 128),
                                      (6, 6, 1241, 376), (9, 5, 200, 150)])
def test_standalone_mid_size_covered_search(S, Wn, w, h):
    """Mid-size grids (and unaligned-width frames) take pixel ranges, give NMI_OPT_SPLIT 0's bits and the model's."""
    wl = sy.workload(w, h, S, Wn, seed=S * 7 + Wn)
    wm, rm = masks_for(S, Wn, w, h, S + Wn)
    rs, ws = wl["render_stack"], wl["warp_stack"]
    got, idx, best, counts, st, cus = covered(rs, ws, wm, rm, wl["bottom_up"])
    if cus == 256 or w % 16:
        assert st["last_launch_ranges"] >= 2, st        # the covered pixel-range kernel ran
    assert st["healed"] == 0
    ref, ri, rb, rc, st0, _ = covered(rs, ws, wm, rm, wl["bottom_up"], {capi.NmiContext.OPT_SPLIT: 0})
    assert st0["last_launch_ranges"] == 0                # the covered grid kernel
    assert (bits(got) == bits(ref)).all() and (idx, bits(best)) == (ri, bits(rb)) and (counts == rc).all()
    if S * Wn * w * h <= 81 * 160 * 128:
        want, wi, wb, wc = cnp.covered_search(rs, ws, wm, rm, render_bottom_up=wl["bottom_up"])
        assert (bits(got) == bits(want)).all() and (idx, bits(best)) == (wi, bits(wb))
        assert (counts == wc).all()
    else:
        assert (counts == cnp.cover_counts(wm, rm, wl["bottom_up"])).all()


@pytest.mark.parametrize("ranges", [2, 3, 4, 5])
def test_forced_ranges_and_background_rule_off(ranges):
    """NMI_OPT_SPLIT 1 + NMI_OPT_SPLIT_PIXELS P forces P ranges; the background rule off at 256 bins (row / column 0 cleared)
    and on give the model's bits; nmi_last_cover_counts holds len[w][s] after the pixel-range launch."""
    w, h, S, Wn = 160, 128, 5, 4
    wl = sy.workload(w, h, S, Wn, seed=ranges)
    wm, rm = masks_for(S, Wn, w, h, ranges)
    rs, ws = wl["render_stack"], wl["warp_stack"]
    rs[:, :10] = 0                                       # raw zeros: the background rule has something to drop
    opts = {capi.NmiContext.OPT_SPLIT: 1, capi.NmiContext.OPT_SPLIT_PIXELS: ranges}
    for use_bg in (True, False):
        got, idx, best, counts, st, _ = covered(rs, ws, wm, rm, wl["bottom_up"], opts, use_bg)
        assert st["last_launch_ranges"] == ranges and st["healed"] == 0
        want, wi, wb, wc = cnp.covered_search(rs, ws, wm, rm, use_bg=use_bg, render_bottom_up=wl["bottom_up"])
        assert (bits(got) == bits(want)).all() and (idx, bits(best)) == (wi, bits(wb)), use_bg
        assert (counts == wc).all()


def wrap_stacks(w, h):
    yy, xx = np.mgrid[0:h, 0:w]
    a = np.where((xx + yy) % 2 == 0, 10, 200).astype(np.uint8)
    b = np.where((xx // 2 + yy) % 2 == 0, 30, 90).astype(np.uint8)
    c = np.where(xx % 7 == 0, 30, 90).astype(np.uint8)
    rs = np.stack([a, np.where(xx % 3 == 0, 10, 200).astype(np.uint8)] * 16)[:32]
    return rs, np.stack([b, c])


def test_counter_wraps_heal_in_the_covered_pixel_range_kernel():
    """Bins of ~70,000 hits under masks that keep most pixels wrap in helpers, owners and merges; the count test (decoded total
    != len) sends those candidates to the covered exact path inside the launch: the same bits, healed > 0 -- and exactly the
    candidates with a bin above 65,535 in the owner's share of the covered pixels or in the helpers' shares together
    (tests/helpers/pix_ranges_np.py), all of them count-test redos, none a timeout."""
    w, h = 640, 480
    rs, ws = wrap_stacks(w, h)
    wm = np.ones((2, h, w), np.uint8)
    wm[0, h - 30:] = 0
    wm[1, :, :11] = 0
    rm = np.ones((32, h, w), np.uint8)
    rm[1::2, :, 600:] = 0
    want, wi, wb, wc = cnp.covered_search(rs, ws, wm, rm, render_bottom_up=False)
    j, _, _ = mnp.masked_hist(rs[0], ws[0], cnp.pair_mask(wm[0], rm[0], False).astype(np.uint8), render_bottom_up=False)
    assert j.max() > 65535  # (the premise)
    for ranges in (2, 3, 4):
        opts = {capi.NmiContext.OPT_SPLIT: 1, capi.NmiContext.OPT_SPLIT_PIXELS: ranges}
        got, idx, best, counts, st, _ = covered(rs, ws, wm, rm, False, opts)
        assert st["last_launch_ranges"] == ranges and st["healed"] > 0, st
        redos = prn.count_test_redos(rs, ws, ranges, False, keep=lambda v, s: cnp.pair_mask(wm[v], rm[s], False))
        assert redos > 0 and (st["healed"], st["timeouts"], st["count_test"]) == (redos, 0, redos), (st, redos)
        assert (idx, bits(best)) == (wi, bits(wb)), ranges
        assert (bits(got) == bits(want)).all(), ranges
        assert (counts == wc).all()


def test_a_missing_helper_is_healed_inside_the_launch():
    """Phase-mask bit 9 (test hook): helper 1 of every candidate withholds its flags, so every owner gives up after its bounded
    wait and scores the candidate alone on the covered exact path -- inside the one launch, with the model's bits.  The next
    call finds that launch's stale blocks (an old tag) and stays exact."""
    w, h, S, Wn = 160, 128, 9, 5
    wl = sy.workload(w, h, S, Wn, seed=3)
    wm, rm = masks_for(S, Wn, w, h, 4)
    want, wi, wb, wc = cnp.covered_search(wl["render_stack"], wl["warp_stack"], wm, rm, render_bottom_up=wl["bottom_up"])
    rs, ws, dwm, drm = dev(wl["render_stack"]), dev(wl["warp_stack"]), dev(wm), dev(rm)
    with capi.NmiContext(w, h, render_bottom_up=wl["bottom_up"]) as ctx:
        ctx.set_option(ctx.OPT_SPLIT, 1)
        ctx.set_option(ctx.OPT_SPLIT_PIXELS, 3)
        assert ctx.search_grid_covered(rs, drm, ws, dwm) == (wi, wb)
        assert ctx.pix_status() == {"last_launch_ranges": 3, "healed": 0}
        assert ctx.pix_heal_counts() == {"timeouts": 0, "count_test": 0}
        ctx.set_option(ctx.OPT_PHASE_MASK, 3 | 512)
        t = torch.zeros((Wn, S), device="cuda")
        t0 = time.perf_counter()
        assert ctx.search_grid_covered(rs, drm, ws, dwm, t) == (wi, wb)
        assert time.perf_counter() - t0 < 0.5
        assert (bits(t.cpu().numpy()) == bits(want)).all()
        assert (ctx.cover_counts(S * Wn).reshape(Wn, S) == wc).all()
        assert ctx.pix_status() == {"last_launch_ranges": 3, "healed": S * Wn}
        assert ctx.pix_heal_counts() == {"timeouts": S * Wn, "count_test": 0}
        ctx.set_option(ctx.OPT_PHASE_MASK, 3)
        assert ctx.search_grid_covered(rs, drm, ws, dwm, t) == (wi, wb)
        assert (bits(t.cpu().numpy()) == bits(want)).all()
        assert ctx.pix_status()["healed"] == S * Wn
        assert ctx.pix_heal_counts() == {"timeouts": S * Wn, "count_test": 0}


def test_empty_and_all_ones_masks():
    """len = 0 scores 0.0; all-ones masks on both sides give nmi_search_grid's bits -- on the pixel-range kernel."""
    w, h, S, Wn = 160, 128, 9, 9
    wl = sy.workload(w, h, S, Wn, seed=9)
    rs, ws = wl["render_stack"], wl["warp_stack"]
    ones_w, ones_r = np.ones((Wn, h, w), np.uint8), np.ones((S, h, w), np.uint8)
    with capi.NmiContext(w, h, render_bottom_up=wl["bottom_up"]) as ctx:
        t_ref = torch.zeros((Wn, S), device="cuda")
        ref = ctx.search_grid(dev(rs), dev(ws), t_ref)
    got, idx, best, counts, st, cus = covered(rs, ws, ones_w, ones_r, wl["bottom_up"])
    if cus == 256:
        assert st["last_launch_ranges"] >= 2
    assert (idx, bits(best)) == (ref[0], bits(ref[1]))
    assert (bits(got) == bits(t_ref.cpu().numpy())).all()
    assert (counts == w * h).all()
    # warp 2 empty, render 4 empty, and a warp / render pair whose masks do not meet
    wm, rm = ones_w.copy(), ones_r.copy()
    wm[2] = 0
    rm[4] = 0
    wm[5, :, : w // 2] = 0
    rm[6, :, w // 2:] = 0
    got, idx, best, counts, st, _ = covered(rs, ws, wm, rm, wl["bottom_up"])
    want, wi, wb, wc = cnp.covered_search(rs, ws, wm, rm, render_bottom_up=wl["bottom_up"])
    assert (counts == wc).all() and counts[2].max() == 0 and counts[:, 4].max() == 0 and counts[5, 6] == 0
    assert (got[2] == 0).all() and (got[:, 4] == 0).all() and got[5, 6] == 0
    assert (bits(got) == bits(want)).all() and (idx, bits(best)) == (wi, bits(wb))
