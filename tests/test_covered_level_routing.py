"""GPU tests (-m gpu): which search kernel a covered level's graph runs.  The covered grid kernel and the covered pixel-range
kernel give the same bits, so the bit comparisons of tests/test_covered_level.py cannot tell them apart; what tells them apart is
the pixel-range kernel's heal counter (nmi_pix_status().healed), which only it counts into: under phase-mask bit 9 (the hand-off
test hook, read when the graph is captured) every candidate of a pixel-range launch heals, and a counter that wraps in a range
heals its candidate.  Each count is read right after the level's replay, before any standalone search runs."""
import numpy as np
import pytest

from helpers import covered_np as cnp
from orbslam2_nmi_amd import capi
from test_covered_level import CoveredScene, bits, dev, hood_mask, views, warps

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def nmi():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    import orbslam2_nmi_amd as m
    m.load_library()
    return m


@pytest.mark.parametrize("mesh", [False, True], ids=["cloud", "mesh"])
@pytest.mark.parametrize("w,h,S,Wn,ranges", [(160, 128, 9, 9, True), (1241, 376, 3, 3, True), (160, 120, 27, 27, False)],
                         ids=["81-candidates", "1241x376", "729-candidates"])
def test_covered_level_search_kernel_by_grid_size(nmi, mesh, w, h, S, Wn, ranges):
    """With bit 9 set when the graph is captured, one replay of a mid-size (or unaligned-row) covered level heals every candidate
    -- the pixel-range kernel ran, its helpers withheld their hand-offs and every owner scored alone, with the model's bits; a
    729-candidate level heals none (the covered grid kernel)."""
    with nmi.NmiContext(w, h) as ctx:
        if ctx.info()["compute_units"] != 256 and w % 16 == 0:
            pytest.skip("the mid-size routing is stated for 256 compute units")
        sc = CoveredScene(nmi, ctx, w, h, mesh)
        fm = dev(hood_mask(w, h))
        ctx.set_option(ctx.OPT_PHASE_MASK, 3 | 512)
        with sc.level(S, Wn) as lv:
            lv.set_coverage(True, fm)
            mvps, Ms = views(sc.rp, S), warps(w, h, Wn)
            win = lv.run(mvps, Ms)
            healed = ctx.pix_status()["healed"]
            assert healed == (S * Wn if ranges else 0)
            rs, ws, t = lv.outputs()
            rm, wm, cnt = lv.coverage()
            assert 0 < np.count_nonzero(rm) < rm.size
            if S * Wn <= 81:
                ro, io, bo, co = cnp.covered_search(rs, ws, wm, rm)
                assert (bits(ro) == bits(t)).all() and win == (io, bo) and (co == cnt).all()
            # hook off again: the graph keeps what it was captured with until coverage is set again
            ctx.set_option(ctx.OPT_PHASE_MASK, 3)
            lv.set_coverage(True, fm)
            assert lv.run(mvps, Ms) == win
            assert ctx.pix_status()["healed"] == healed
            assert (bits(lv.outputs()[2]) == bits(t)).all()


@pytest.mark.parametrize("S,Wn,ranges", [(9, 9, True), (27, 27, False)], ids=["pixel-ranges", "grid-kernel"])
def test_counter_wraps_heal_in_the_covered_level(nmi, S, Wn, ranges):
    """A flat frame and a one-colour cloud at 640x480: one joint bin holds nearly every covered pixel, more than 65,535 in every
    range.  The mid-size level's pixel-range kernel heals those candidates inside the launch (healed > 0); the 729-candidate
    level's grid kernel redoes them in its exact launch, which the heal counter does not count.  Both give the model's bits."""
    from test_render import plane_cloud
    w, h = 640, 480
    xyz, red, rp = plane_cloud(w, h, density=1.2)
    u = xyz[:, 0] / xyz[:, 2] * rp.fx + rp.cx
    keep = ~((u >= 0.4 * w) & (u < 0.5 * w))
    with nmi.NmiContext(w, h) as ctx:
        dx, dr = dev(xyz[keep]), dev(np.full_like(red[keep], 0.5))
        frame = dev(np.full((h, w), 100, np.uint8))
        with nmi.NmiLevel(ctx, dx, dr, frame, S, Wn, 3.0) as lv:
            lv.set_coverage(True)
            mvps, Ms = views(rp, S), warps(w, h, Wn)
            win = lv.run(mvps, Ms)
            healed = ctx.pix_status()["healed"]
            assert (healed > 0) if ranges else (healed == 0)
            rs, ws, t = lv.outputs()
            rm, wm, cnt = lv.coverage()
            t2 = torch.full(t.shape, -3.0, device="cuda")
            assert ctx.search_grid_covered(dev(rs), dev(rm), dev(ws), dev(wm), t2) == win
            assert (bits(t2.cpu().numpy()) == bits(t)).all()
            if ranges:
                ro, io, bo, co = cnp.covered_search(rs, ws, wm, rm)
                assert (bits(ro) == bits(t)).all() and win == (io, bo) and (co == cnt).all()
