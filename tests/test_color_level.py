"""GPU tests (-m gpu) of coloured levels (nmi_level_set_frame_format).

The contract: a level whose frame is a colour (or pitched) camera frame equals the standalone chain on that frame --
nmi_gray_frame -> [nmi_undistort_frame] -> nmi_warp_stack[_masked] -> render -> nmi_search_grid[_masked / _covered] -- on == of
ratings bits, winner, warps, warp masks and coverage.  Also: blocks compose to the level and an RCCL run at world size 1 gives
its winner, the frame is read in place on every replay, masks / coverage / distortion set in either order keep the format, and
turning it off gives the bytes of a never-formatted level."""
import numpy as np
import pytest

from helpers import color_np as cnp
from helpers import undistort_np as unp
from orbslam2_nmi_amd import capi, sharding
from test_covered_level import CoveredScene
from test_masked_level import Scene, compose, dev, hood_mask, views, warps

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

LENSES = {"none": None, "barrel": unp.FAMILIES["barrel"], "pincushion": unp.FAMILIES["pincushion"]}


@pytest.fixture(scope="module")
def nmi():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    import orbslam2_nmi_amd as m
    m.load_library()
    return m


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def lens_K(rp):
    return np.array([[rp.fx, 0, rp.cx], [0, rp.fy, rp.cy], [0, 0, 1.0]])


class ColorFrame:
    """The scene's grey frame coloured (helpers/color_np.py: colorize) and laid out in fmt with a pitch, `off` bytes into a device
    allocation.  .view is the frame's first byte onwards: the level's d_frame."""

    def __init__(self, sc, fmt, pitch, off, seed=0):
        self.fmt, self.pitch, self.off = fmt, pitch, off
        self.w, self.h = sc.w, sc.h
        self.rgb = cnp.colorize(sc.frame.cpu().numpy(), seed)
        self.buf = dev(cnp.pack(self.rgb, fmt, pitch, off, seed=seed))
        self.view = self.buf[off:]

    def refill(self, rgb, seed):
        """New contents in place (the same addresses)."""
        self.rgb = rgb
        self.buf.copy_(dev(cnp.pack(rgb, self.fmt, self.pitch, self.off, seed=seed)))
        torch.cuda.synchronize()


def level(nmi, sc, cf, S, Wn, block=None):
    return nmi.NmiLevel(sc.ctx, sc.dx, sc.da, cf.view, S, Wn, 3.0, texture=sc.tex, block=block)


def chain(ctx, sc, cf, kind, K, dist, fm, mvps, Ms, rs):
    """The standalone chain on the colour frame -> (winner, ratings, warps, warp masks or None)."""
    gray = ctx.gray_frame(cf.view, cf.fmt, cf.pitch)
    assert (gray.cpu().numpy() == cnp.to_gray(cf.buf.cpu().numpy(), cf.fmt, cf.w, cf.h, cf.pitch, cf.off)).all()
    t2 = torch.full((len(Ms), len(mvps)), -3.0, device="cuda")
    if kind == "plain":
        frame = gray if dist is None else ctx.undistort_frame(gray, K, dist, out_mask=False)[0]
        ws = ctx.warp_stack(frame, Ms)
        win = ctx.search_grid(dev(rs), ws, t2)
        return win, t2.cpu().numpy(), ws.cpu().numpy(), None
    frame, fmask = (gray, fm) if dist is None else ctx.undistort_frame(gray, K, dist, raw_mask=fm)
    ws, wm = ctx.warp_stack_masked(frame, Ms, fmask)
    if kind == "masked":
        win = ctx.search_grid_masked(dev(rs), ws, wm, t2)
    else:
        rs2, rm2 = sc.chain_renders(ctx, mvps)
        assert (rs2.cpu().numpy() == rs).all()
        win = ctx.search_grid_covered(rs2, rm2, ws, wm, t2)
    return win, t2.cpu().numpy(), ws.cpu().numpy(), wm.cpu().numpy()


def check(ctx, sc, cf, lv, kind, K, dist, fm, mvps, Ms):
    win = lv.run(mvps, Ms)
    rs, ws, t = lv.outputs()
    cw, ct, cws, cwm = chain(ctx, sc, cf, kind, K, dist, fm, mvps, Ms, rs)
    assert (cws == ws).all(), "level warps != warps of the converted frame"
    assert cw == win and (bits(ct) == bits(t)).all(), (cw, win)
    if kind == "masked":
        wm, cnt = lv.masks()
        assert (wm == cwm).all()
        assert (cnt == np.count_nonzero(cwm.reshape(len(Ms), -1), axis=1)).all()
    if kind == "covered":
        rm, wm, cnt = lv.coverage()
        assert (wm == cwm).all()
    return win, t


def scene(nmi, ctx, w, h, mesh, kind):
    return CoveredScene(nmi, ctx, w, h, mesh) if kind == "covered" else Scene(nmi, ctx, w, h, mesh)


def enable(lv, kind, fm):
    if kind == "masked":
        lv.set_masks(True, fm)
    elif kind == "covered":
        lv.set_coverage(True, fm)


CASES = [(640, 480, cnp.RGB, 0, 0), (1241, 376, cnp.BGRA, 1241 * 4 + 5, 3)]   # dense / odd width, odd pitch, unaligned base


@pytest.mark.parametrize("lens", list(LENSES))
@pytest.mark.parametrize("kind", ["plain", "masked", "covered"])
@pytest.mark.parametrize("mesh", [False, True], ids=["cloud", "mesh"])
@pytest.mark.parametrize("case", CASES, ids=["640x480-rgb", "1241x376-bgra-pitched"])
def test_colored_level_equals_the_chain(nmi, case, mesh, kind, lens):
    """Format set before and after the masks (and the distortion); replays with changed views and warps; the colour frame's
    contents replaced in place."""
    w, h, fmt, pitch, off = case
    S, Wn = 3, 3
    dist = LENSES[lens]
    with nmi.NmiContext(w, h) as ctx:
        sc = scene(nmi, ctx, w, h, mesh, kind)
        K = lens_K(sc.rp)
        cf = ColorFrame(sc, fmt, pitch, off)
        fm = dev(hood_mask(w, h)) if kind != "plain" else None
        mvps, Ms = views(sc.rp, S), warps(w, h, Wn)
        with level(nmi, sc, cf, S, Wn) as lv, level(nmi, sc, cf, S, Wn) as lv2:
            lv.set_frame_format(fmt, pitch)            # format first, then distortion and masks
            if dist is not None:
                lv.set_distortion(K, dist)
            enable(lv, kind, fm)
            enable(lv2, kind, fm)                      # masks and distortion first, then the format
            if dist is not None:
                lv2.set_distortion(K, dist)
            lv2.set_frame_format(fmt, pitch)
            first = check(ctx, sc, cf, lv, kind, K, dist, fm, mvps, Ms)
            again = check(ctx, sc, cf, lv2, kind, K, dist, fm, mvps, Ms)
            assert again[0] == first[0] and (bits(again[1]) == bits(first[1])).all()
            check(ctx, sc, cf, lv, kind, K, dist, fm, views(sc.rp, S, 1.7), warps(w, h, Wn, 1.6))
            cf.refill(np.roll(cf.rgb, shift=(7, 11), axis=(0, 1)), seed=1)   # the frame changes in place
            if fm is not None:
                fm[h // 3:h // 2, w // 3:w // 2] = 0
                torch.cuda.synchronize()
            check(ctx, sc, cf, lv, kind, K, dist, fm, mvps, Ms)


@pytest.mark.parametrize("kind", ["plain", "masked"])
def test_colored_blocks_compose_to_the_level(nmi, kind):
    w, h, S, Wn = 640, 480, 4, 3
    with nmi.NmiContext(w, h) as ctx:
        sc = Scene(nmi, ctx, w, h, False)
        K = lens_K(sc.rp)
        cf = ColorFrame(sc, cnp.BGR, 640 * 3 + 64, 1)
        fm = dev(hood_mask(w, h)) if kind == "masked" else None
        mvps, Ms = views(sc.rp, S), warps(w, h, Wn)
        dist = LENSES["barrel"]
        with level(nmi, sc, cf, S, Wn) as full:
            full.set_frame_format(cf.fmt, cf.pitch)
            full.set_distortion(K, dist)
            enable(full, kind, fm)
            ref, t_ref = check(ctx, sc, cf, full, kind, K, dist, fm, mvps, Ms)
            got = []
            for rank in range(2):
                so, sc_, wo, wc = sharding.grid_shard(S, Wn, rank, 2)
                with level(nmi, sc, cf, sc_, wc, block=(so, S, wo, Wn)) as blk:
                    enable(blk, kind, fm)
                    blk.set_distortion(K, dist)
                    blk.set_frame_format(cf.fmt, cf.pitch)
                    got.append(blk.run(mvps[so:so + sc_], Ms[wo:wo + wc]))
                    _, ws, t = blk.outputs()
                    assert (bits(t) == bits(t_ref[wo:wo + wc, so:so + sc_])).all()
            assert compose(got) == ref
            with level(nmi, sc, cf, 0, Wn, block=(S, S, 0, Wn)) as empty, level(nmi, sc, cf, S, Wn, block=(0, S, 0, Wn)) as whole:
                empty.set_frame_format(cf.fmt, cf.pitch)          # an empty block takes the setting and has no node
                whole.set_frame_format(cf.fmt, cf.pitch)
                for lv in (empty, whole):
                    lv.set_distortion(K, dist)
                    enable(lv, kind, fm)
                assert empty.run(mvps[:0], Ms) == (-1, np.float32(0))
                comm = ctx.rccl_comm_init(capi.rccl_unique_id(), 0, 1)   # nmi_level_run_rccl at world size 1
                try:
                    assert empty.run_rccl(mvps[:0], Ms, comm) == (-1, np.float32(0))
                    assert whole.run_rccl(mvps, Ms, comm) == ref
                    assert (bits(whole.outputs()[2]) == bits(t_ref)).all()
                finally:
                    capi.rccl_comm_destroy(comm)


@pytest.mark.parametrize("mesh", [False, True], ids=["cloud", "mesh"])
def test_format_off_is_the_never_formatted_level(nmi, mesh):
    """(GRAY, 0) and (GRAY, W) restore the graph: bytes == a level on the same buffer that never had a format, with and without
    distortion; toggling masks and coverage in between keeps the format.  Rejected calls leave the level as it was."""
    w, h, S, Wn = 848, 480, 3, 3
    with nmi.NmiContext(w, h) as ctx:
        sc = CoveredScene(nmi, ctx, w, h, mesh)
        K = lens_K(sc.rp)
        cf = ColorFrame(sc, cnp.RGBA, 0, 0)
        mvps, Ms = views(sc.rp, S), warps(w, h, Wn)
        lens = LENSES["pincushion"]
        with level(nmi, sc, cf, S, Wn) as lv, level(nmi, sc, cf, S, Wn) as never, level(nmi, sc, cf, S, Wn) as never_d:
            never_d.set_distortion(K, lens)
            refs = {}
            for name, ref in (("plain", never), ("distorted", never_d)):
                refs[name] = (ref.run(mvps, Ms), ref.outputs())

            def same_as(name):
                win, out = refs[name]
                assert lv.run(mvps, Ms) == win
                for a, b in zip(lv.outputs(), out):
                    assert (np.ascontiguousarray(a).view(np.uint8) == np.ascontiguousarray(b).view(np.uint8)).all()

            lv.set_frame_format(cnp.RGBA, 0)
            check(ctx, sc, cf, lv, "plain", K, None, None, mvps, Ms)
            for bad in ((9, 0), (cnp.RGBA, 1), (cnp.RGBA, w * 4 - 1), (cnp.RGB, -3)):
                with pytest.raises(capi.NmiError):
                    lv.set_frame_format(*bad)
            check(ctx, sc, cf, lv, "plain", K, None, None, mvps, Ms)      # as it was
            lv.set_masks(True)
            check(ctx, sc, cf, lv, "masked", K, None, None, mvps, Ms)
            lv.set_masks(False)
            lv.set_coverage(True)
            check(ctx, sc, cf, lv, "covered", K, None, None, mvps, Ms)
            lv.set_coverage(False)
            lv.set_frame_format(cnp.GRAY, 0)
            same_as("plain")
            lv.set_frame_format(cnp.RGBA, 0)
            lv.set_distortion(K, lens)
            check(ctx, sc, cf, lv, "plain", K, lens, None, mvps, Ms)
            lv.set_frame_format(cnp.GRAY, w)
            same_as("distorted")
            lv.set_frame_format(cnp.RGBA, 0)
            lv.set_distortion(None, None)                                  # distortion off keeps the format
            check(ctx, sc, cf, lv, "plain", K, None, None, mvps, Ms)
            lv.set_frame_format(cnp.GRAY, 0)
            same_as("plain")
