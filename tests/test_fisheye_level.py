"""GPU tests (-m gpu) of fisheye levels (nmi_level_set_distortion_fisheye), with the harness of tests/test_undistort_level.py.

The contract: a fisheye level's replay equals the standalone chain on the raw frame -- nmi_undistort_frame_fisheye ->
nmi_warp_stack (plain), -> nmi_warp_stack_masked on the undistorted frame and mask (masked), with coverage (covered) -- on ==
of ratings bits, winner, warps and masks, and that chain's ratings equal the CPU oracle on the device's warps.  Also: with a
frame reduction the lens applies to the reduced frame; a level has one lens setting (of the two setters the later call wins,
NULL in either turns it off, four zero coefficients do not); blocks compose to the level; and a masked fisheye level recovers
a planted pose from a render seen through the lens (tests/helpers/fisheye_np.py: fisheye_image), which the same level without
the lens setting does not."""
import numpy as np
import pytest

from helpers import fisheye_np as fnp
from helpers import undistort_np as unp
from orbslam2_nmi_amd import capi, sharding
from test_covered_level import CoveredScene
from test_masked_level import Scene, camera, compose, dev, hood_mask, views, warps
from test_undistort_level import bits, check, enable, lens_K, scene

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

LENS = fnp.FAMILIES["euroc_eq"]
RADTAN = unp.FAMILIES["pincushion"]
SHAPES = [(640, 480, 3, 3), (1241, 376, 3, 3)]   # rows of 16-byte chunks (fused fronts) and not (byte paths, side-branch warp)


@pytest.fixture(scope="module")
def nmi():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    import orbslam2_nmi_amd as m
    m.load_library()
    return m


def raw_K(K, w):
    """The raw camera of a level whose renders use K: a longer focal length (K is K_raw scaled by 0.6, a wider pinhole view
    with an invalid border) and the principal point off K's."""
    Kr = fnp.pinhole_K(K, 1 / 0.6)
    Kr[0, 2] += 0.02 * w
    Kr[1, 2] -= 0.01 * w
    return Kr


@pytest.mark.parametrize("kind", ["plain", "masked", "covered"])
@pytest.mark.parametrize("shape,mesh", [(SHAPES[0], False), (SHAPES[1], False), (SHAPES[0], True)],
                         ids=["640x480-cloud", "1241x376-cloud", "640x480-mesh"])
def test_fisheye_level_equals_the_chain(nmi, shape, mesh, kind):
    """The lens set before and after the masks; replays with changed views and warps; the raw frame's contents replaced."""
    w, h, S, Wn = shape
    with nmi.NmiContext(w, h) as ctx:
        sc = scene(nmi, ctx, w, h, mesh, kind)
        K = lens_K(sc.rp)
        Kr = raw_K(K, w)
        fctx = fnp.FisheyeCtx(ctx, Kr)
        fm = dev(hood_mask(w, h)) if kind != "plain" else None
        mvps, Ms = views(sc.rp, S), warps(w, h, Wn)
        with sc.level(S, Wn) as lv, sc.level(S, Wn) as lv2:
            lv.set_distortion_fisheye(K, Kr, LENS)        # the lens first, then the masks
            enable(lv, kind, fm)
            enable(lv2, kind, fm)                          # masks first, then the lens
            lv2.set_distortion_fisheye(K, Kr, LENS)
            first = check(fctx, sc, lv, kind, K, LENS, fm, mvps, Ms)
            again = check(fctx, sc, lv2, kind, K, LENS, fm, mvps, Ms, oracle=False)
            assert again[0] == first[0] and (bits(again[1]) == bits(first[1])).all()
            check(fctx, sc, lv, kind, K, LENS, fm, views(sc.rp, S, 1.7), warps(w, h, Wn, 1.6), oracle=False)
            sc.frame.copy_(torch.roll(sc.frame, shifts=(7, 11), dims=(0, 1)))  # the raw frame changes in place
            if fm is not None:
                fm[h // 3:h // 2, w // 3:w // 2] = 0
            torch.cuda.synchronize()
            moved = check(fctx, sc, lv, kind, K, LENS, fm, mvps, Ms, oracle=False)
            assert (bits(moved[1]) != bits(first[1])).any()
            # the premise: the chain's frame is the twin's, with an invalid border
            ef, em = fnp.undistort(sc.frame.cpu().numpy(), K, Kr, LENS)
            ud, udm = ctx.undistort_frame_fisheye(sc.frame, K, Kr, LENS)
            assert (ud.cpu().numpy() == ef).all() and (udm.cpu().numpy() == em).all() and 0 < em.sum() < w * h


def test_fisheye_level_with_frame_reduction(nmi):
    """nmi_level_set_frame_reduction factor 2 with the lens set == reduce -> undistort (K, K_raw of the reduced frame) -> chain,
    whichever is set first."""
    from helpers import color_np as cnp
    from test_reduce_level import FullFrame, level
    from test_reduce_level import check as rcheck
    w, h, f, S, Wn = 424, 240, 2, 3, 3
    with nmi.NmiContext(w, h) as ctx:
        sc = Scene(nmi, ctx, w, h, False)
        K = lens_K(sc.rp)
        Kr = raw_K(K, w)
        fctx = fnp.FisheyeCtx(ctx, Kr)
        ff = FullFrame(sc, f, cnp.RGB, f * w * 3 + 16, 0)
        fm = dev(hood_mask(w, h))
        mvps, Ms = views(sc.rp, S), warps(w, h, Wn)
        with level(nmi, sc, ff, S, Wn) as lv, level(nmi, sc, ff, S, Wn) as lv2:
            lv.set_frame_reduction(ff.f, ff.fmt, ff.pitch)
            lv.set_distortion_fisheye(K, Kr, LENS)
            lv.set_masks(True, fm)
            lv2.set_masks(True, fm)
            lv2.set_distortion_fisheye(K, Kr, LENS)
            lv2.set_frame_reduction(ff.f, ff.fmt, ff.pitch)
            first = rcheck(fctx, sc, ff, lv, "masked", K, LENS, fm, mvps, Ms)
            again = rcheck(fctx, sc, ff, lv2, "masked", K, LENS, fm, mvps, Ms)
            assert again[0] == first[0] and (bits(again[1]) == bits(first[1])).all()
            lv.set_masks(False)
            rcheck(fctx, sc, ff, lv, "plain", K, LENS, None, mvps, Ms)


@pytest.mark.parametrize("order", ["radtan-first", "fisheye-first"])
def test_one_lens_setting_the_later_call_wins(nmi, order):
    """Radial-tangential, then fisheye, then off -- and the other order -- give in turn the bytes of a level of that lens and of
    a never-distorted level; NULL through either setter turns either lens off; four zero coefficients are still a lens."""
    w, h, S, Wn = 848, 480, 3, 3
    with nmi.NmiContext(w, h) as ctx:
        sc = CoveredScene(nmi, ctx, w, h, False)
        K = lens_K(sc.rp)
        Kr = raw_K(K, w)
        fctx = fnp.FisheyeCtx(ctx, Kr)
        mvps, Ms = views(sc.rp, S), warps(w, h, Wn)
        with sc.level(S, Wn) as lv, sc.level(S, Wn) as never, sc.level(S, Wn) as only_r, sc.level(S, Wn) as only_f:
            only_r.set_distortion(K, RADTAN)
            only_f.set_distortion_fisheye(K, Kr, LENS)
            refs = {name: (ref.run(mvps, Ms), ref.outputs()) for name, ref in (("never", never), ("radtan", only_r), ("fisheye", only_f))}
            assert (refs["radtan"][1][1] != refs["fisheye"][1][1]).any() and (refs["never"][1][1] != refs["fisheye"][1][1]).any()

            def same_as(name):
                win, out = refs[name]
                assert lv.run(mvps, Ms) == win
                for a, b in zip(lv.outputs(), out):
                    assert (np.ascontiguousarray(a).view(np.uint8) == np.ascontiguousarray(b).view(np.uint8)).all(), name

            def radtan():
                lv.set_distortion(K, RADTAN)
                check(ctx, sc, lv, "plain", K, RADTAN, None, mvps, Ms, oracle=False)
                same_as("radtan")

            def fisheye():
                lv.set_distortion_fisheye(K, Kr, LENS)
                check(fctx, sc, lv, "plain", K, LENS, None, mvps, Ms, oracle=False)
                same_as("fisheye")

            if order == "radtan-first":
                radtan()
                fisheye()
                lv.set_distortion_fisheye(None, None, None)   # off through the fisheye setter
                same_as("never")
                radtan()
                lv.set_distortion_fisheye(None, None, None)   # ... which also turns the other lens off
                same_as("never")
            else:
                fisheye()
                radtan()
                lv.set_distortion(None, None)
                same_as("never")
                fisheye()
                lv.set_distortion(None, None)                 # off through the other setter
                same_as("never")
                fisheye()
                lv.set_distortion(K, np.zeros(5))             # five zero coefficients: radial-tangential identity, off
                same_as("never")
            lv.set_masks(True)                                # masks keep the lens, and a refused call changes nothing
            lv.set_distortion_fisheye(K, None, np.zeros(4))   # an ideal equidistant lens with K_raw = K: still a remap
            with pytest.raises(capi.NmiError):
                lv.set_distortion_fisheye(K, Kr * 0, LENS)
            with pytest.raises(capi.NmiError):
                lv.set_distortion_fisheye(K, Kr, (0.1, np.nan, 0, 0))
            check(fnp.FisheyeCtx(ctx, None), sc, lv, "masked", K, np.zeros(4), None, mvps, Ms, oracle=False)
            assert (lv.outputs()[1] != refs["never"][1][1]).any()
            lv.set_masks(False)
            lv.set_distortion_fisheye(None, None, None)
            same_as("never")


@pytest.mark.parametrize("kind", ["plain", "masked"])
def test_fisheye_blocks_compose_to_the_level(nmi, kind):
    w, h, S, Wn = 640, 480, 4, 3
    with nmi.NmiContext(w, h) as ctx:
        sc = Scene(nmi, ctx, w, h, False)
        K = lens_K(sc.rp)
        Kr = raw_K(K, w)
        fctx = fnp.FisheyeCtx(ctx, Kr)
        fm = dev(hood_mask(w, h)) if kind == "masked" else None
        mvps, Ms = views(sc.rp, S), warps(w, h, Wn)
        with sc.level(S, Wn) as full:
            full.set_distortion_fisheye(K, Kr, LENS)
            enable(full, kind, fm)
            ref, t_ref = check(fctx, sc, full, kind, K, LENS, fm, mvps, Ms, oracle=False)
            got = []
            for rank in range(2):
                so, sc_, wo, wc = sharding.grid_shard(S, Wn, rank, 2)
                with sc.level(sc_, wc, block=(so, S, wo, Wn)) as blk:
                    blk.set_distortion_fisheye(K, Kr, LENS)
                    enable(blk, kind, fm)
                    got.append(blk.run(mvps[so:so + sc_], Ms[wo:wo + wc]))
                    _, ws, t = blk.outputs()
                    assert (bits(t) == bits(t_ref[wo:wo + wc, so:so + sc_])).all()
            assert compose(got) == ref
            with sc.level(0, Wn, block=(S, S, 0, Wn)) as empty, sc.level(S, Wn, block=(0, S, 0, Wn)) as whole:
                empty.set_distortion_fisheye(K, Kr, LENS)          # an empty block takes the setting and has no node
                whole.set_distortion_fisheye(K, Kr, LENS)
                enable(empty, kind, fm)
                enable(whole, kind, fm)
                assert empty.run(mvps[:0], Ms) == (-1, np.float32(0))
                comm = ctx.rccl_comm_init(capi.rccl_unique_id(), 0, 1)   # nmi_level_run_rccl at world size 1
                try:
                    assert empty.run_rccl(mvps[:0], Ms, comm) == (-1, np.float32(0))
                    assert whole.run_rccl(mvps, Ms, comm) == ref
                    assert (bits(whole.outputs()[2]) == bits(t_ref)).all()
                finally:
                    capi.rccl_comm_destroy(comm)


def test_masked_fisheye_level_recovers_the_planted_pose(nmi):
    """The camera frame: the pinhole view of the map from a known pose, seen through a fisheye lens (float64 resampler) whose
    principal point lies one warp step beside the pinhole's.  With the lens set, a masked level's winner is the candidate at
    that pose (identity warp), scoring strictly higher there than the same level without the lens, whose winner is another
    cell (the premise: the lens matters)."""
    w, h = 640, 480
    with nmi.NmiContext(w, h) as ctx:
        sc = Scene(nmi, ctx, w, h, False)
        K = lens_K(sc.rp)
        Kr = K.copy()
        Kr[0, 2] += 0.02 * K[0, 0]                        # one step of the warp grid below (0.02 rad about y)
        pinhole = sc.frame.cpu().numpy()                  # rendered from camera() + (0.05, 0, 0)
        sc.frame.copy_(dev(fnp.fisheye_image(pinhole, K, Kr, LENS)))
        torch.cuda.synchronize()
        cam = camera()
        offsets = [(0.05 + dx, dy, 0.0) for dx, dy in ((-0.3, 0), (0, 0), (0.3, 0), (0, 0.3), (0, -0.3))]
        mvps = np.stack([capi.render_mvp(sc.rp, *cam, t) for t in offsets])
        Ms = warps(w, h, 9)                               # 3 x 3 x 1: the identity is warp 4
        S, planted = len(offsets), 4 * len(offsets) + 1
        assert np.allclose(Ms[4], np.eye(3))
        with sc.level(S, 9) as lv:
            lv.set_masks(True)
            win_plain, t_plain = (lv.run(mvps, Ms), lv.outputs()[2])
            lv.set_distortion_fisheye(K, Kr, LENS)
            win, t_dist = check(fnp.FisheyeCtx(ctx, Kr), sc, lv, "masked", K, LENS, None, mvps, Ms, oracle=False)
        print("planted", planted, "with the lens", win, "without", win_plain, t_dist.reshape(-1)[planted], t_plain.reshape(-1)[planted])
        assert win[0] == planted, (win, planted)
        assert win_plain[0] != planted, win_plain
        assert t_dist.reshape(-1)[planted] > t_plain.reshape(-1)[planted], (t_dist.reshape(-1)[planted], t_plain.reshape(-1)[planted])
