"""GPU tests (-m gpu) of distorted levels (nmi_level_set_distortion).

The contract: a distorted level's replay equals the standalone chain on the raw frame -- nmi_undistort_frame -> nmi_warp_stack
(plain), -> nmi_warp_stack_masked on the undistorted frame and mask (masked), with coverage (covered) -- on == of ratings bits,
winner and warps; and that chain's ratings equal the CPU oracle on the device's undistorted warps.  Also: blocks compose to the
level, the raw frame is read in place on every replay, turning distortion off (NULL or zero coefficients) gives the bytes of a
never-distorted level, toggling masks / coverage keeps it, and a masked distorted level recovers a planted pose from a frame
seen through the lens (tests/helpers/undistort_np.py: distort_image)."""
import numpy as np
import pytest

from helpers import covered_np as cnp
from helpers import masked_np as mnp
from helpers import undistort_np as unp
from oracle import binding as oc
from orbslam2_nmi_amd import capi, sharding
from test_covered_level import CoveredScene
from test_masked_level import Scene, camera, compose, dev, hood_mask, views, warps

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

BARREL = unp.FAMILIES["barrel"]
LENS = unp.FAMILIES["pincushion"]   # undistorted corners sample outside the raw frame: an invalid border
SHAPES = [(640, 480, 3, 3), (1241, 376, 3, 3)]   # rows of 16-byte chunks (fused fronts) and not (byte paths, side-branch warp)


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


def chain(ctx, sc, kind, K, dist, fm, mvps, Ms, rs):
    """The standalone chain on the raw frame sc.frame -> (winner, ratings, warps, warp masks or None)."""
    t2 = torch.full((len(Ms), len(mvps)), -3.0, device="cuda")
    if kind == "plain":
        ud, _ = ctx.undistort_frame(sc.frame, K, dist, out_mask=False)
        ws = ctx.warp_stack(ud, Ms)
        win = ctx.search_grid(dev(rs), ws, t2)
        return win, t2.cpu().numpy(), ws.cpu().numpy(), None
    ud, udm = ctx.undistort_frame(sc.frame, K, dist, raw_mask=fm)
    ws, wm = ctx.warp_stack_masked(ud, Ms, udm)
    if kind == "masked":
        win = ctx.search_grid_masked(dev(rs), ws, wm, t2)
    else:
        rs2, rm2 = sc.chain_renders(ctx, mvps)
        assert (rs2.cpu().numpy() == rs).all()
        win = ctx.search_grid_covered(rs2, rm2, ws, wm, t2)
    return win, t2.cpu().numpy(), ws.cpu().numpy(), wm.cpu().numpy()


def check(ctx, sc, lv, kind, K, dist, fm, mvps, Ms, oracle=True):
    win = lv.run(mvps, Ms)
    rs, ws, t = lv.outputs()
    cw, ct, cws, cwm = chain(ctx, sc, kind, K, dist, fm, mvps, Ms, rs)
    assert (cws == ws).all(), "level warps != warps of the undistorted frame"
    assert cw == win and (bits(ct) == bits(t)).all(), (cw, win)
    if kind == "masked":
        assert (lv.masks()[0] == cwm).all()
    if kind == "covered":
        rm, wm, cnt = lv.coverage()
        assert (wm == cwm).all()
    if oracle:
        if kind == "plain":
            with oc.rounded():
                ro, io, bo = oc.search_grid(rs, ws, threads=4)
        elif kind == "masked":
            ro, io, bo = mnp.masked_search(rs, ws, cwm)
        else:
            ro, io, bo, _ = cnp.covered_search(rs, ws, wm, rm)
        assert (bits(ro) == bits(t)).all()
        assert win == (io, bo)
    return win, t


def scene(nmi, ctx, w, h, mesh, kind):
    return CoveredScene(nmi, ctx, w, h, mesh) if kind == "covered" else Scene(nmi, ctx, w, h, mesh)


def enable(lv, kind, fm):
    if kind == "masked":
        lv.set_masks(True, fm)
    elif kind == "covered":
        lv.set_coverage(True, fm)


@pytest.mark.parametrize("kind", ["plain", "masked", "covered"])
@pytest.mark.parametrize("mesh", [False, True], ids=["cloud", "mesh"])
@pytest.mark.parametrize("shape", SHAPES, ids=[f"{s[0]}x{s[1]}" for s in SHAPES])
def test_distorted_level_equals_the_chain(nmi, shape, mesh, kind):
    """Distortion set before and after the masks; replays with changed views and warps; the raw frame's contents replaced."""
    w, h, S, Wn = shape
    with nmi.NmiContext(w, h) as ctx:
        sc = scene(nmi, ctx, w, h, mesh, kind)
        K = lens_K(sc.rp)
        fm = dev(hood_mask(w, h)) if kind != "plain" else None
        mvps, Ms = views(sc.rp, S), warps(w, h, Wn)
        with sc.level(S, Wn) as lv, sc.level(S, Wn) as lv2:
            lv.set_distortion(K, LENS)        # distortion first, then the masks
            enable(lv, kind, fm)
            enable(lv2, kind, fm)               # masks first, then distortion
            lv2.set_distortion(K, LENS)
            first = check(ctx, sc, lv, kind, K, LENS, fm, mvps, Ms)
            again = check(ctx, sc, lv2, kind, K, LENS, fm, mvps, Ms, oracle=False)
            assert again[0] == first[0] and (bits(again[1]) == bits(first[1])).all()
            check(ctx, sc, lv, kind, K, LENS, fm, views(sc.rp, S, 1.7), warps(w, h, Wn, 1.6), oracle=False)
            sc.frame.copy_(torch.roll(sc.frame, shifts=(7, 11), dims=(0, 1)))  # the raw frame changes in place
            if fm is not None:
                fm[h // 3:h // 2, w // 3:w // 2] = 0
            torch.cuda.synchronize()
            check(ctx, sc, lv, kind, K, LENS, fm, mvps, Ms, oracle=False)


@pytest.mark.parametrize("kind", ["plain", "masked"])
def test_distorted_blocks_compose_to_the_level(nmi, kind):
    w, h, S, Wn = 640, 480, 4, 3
    with nmi.NmiContext(w, h) as ctx:
        sc = Scene(nmi, ctx, w, h, False)
        K = lens_K(sc.rp)
        fm = dev(hood_mask(w, h)) if kind == "masked" else None
        mvps, Ms = views(sc.rp, S), warps(w, h, Wn)
        with sc.level(S, Wn) as full:
            full.set_distortion(K, LENS)
            enable(full, kind, fm)
            ref, t_ref = check(ctx, sc, full, kind, K, LENS, fm, mvps, Ms, oracle=False)
            got = []
            for rank in range(2):
                so, sc_, wo, wc = sharding.grid_shard(S, Wn, rank, 2)
                with sc.level(sc_, wc, block=(so, S, wo, Wn)) as blk:
                    blk.set_distortion(K, LENS)
                    enable(blk, kind, fm)
                    got.append(blk.run(mvps[so:so + sc_], Ms[wo:wo + wc]))
                    _, ws, t = blk.outputs()
                    assert (bits(t) == bits(t_ref[wo:wo + wc, so:so + sc_])).all()
            assert compose(got) == ref
            with sc.level(0, Wn, block=(S, S, 0, Wn)) as empty, sc.level(S, Wn, block=(0, S, 0, Wn)) as whole:
                empty.set_distortion(K, LENS)                      # an empty block takes the setting and has no node
                whole.set_distortion(K, LENS)
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


@pytest.mark.parametrize("mesh", [False, True], ids=["cloud", "mesh"])
def test_distortion_off_is_the_never_distorted_level(nmi, mesh):
    """dist = NULL and all-zero coefficients restore the plain graph: bytes == a level that never had distortion; toggling the
    masks and coverage in between keeps distortion."""
    w, h, S, Wn = 848, 480, 3, 3
    with nmi.NmiContext(w, h) as ctx:
        sc = CoveredScene(nmi, ctx, w, h, mesh)
        K = lens_K(sc.rp)
        mvps, Ms = views(sc.rp, S), warps(w, h, Wn)
        with sc.level(S, Wn) as lv, sc.level(S, Wn) as never:
            wn_ref = never.run(mvps, Ms)
            out_ref = never.outputs()

            def same_as_never():
                assert lv.run(mvps, Ms) == wn_ref
                for a, b in zip(lv.outputs(), out_ref):
                    assert (np.ascontiguousarray(a).view(np.uint8) == np.ascontiguousarray(b).view(np.uint8)).all()

            lv.set_distortion(K, LENS)
            check(ctx, sc, lv, "plain", K, LENS, None, mvps, Ms, oracle=False)
            lv.set_masks(True)
            check(ctx, sc, lv, "masked", K, LENS, None, mvps, Ms, oracle=False)
            lv.set_masks(False)
            check(ctx, sc, lv, "plain", K, LENS, None, mvps, Ms, oracle=False)
            lv.set_coverage(True)
            check(ctx, sc, lv, "covered", K, LENS, None, mvps, Ms, oracle=False)
            lv.set_coverage(False)
            lv.set_distortion(None, None)
            same_as_never()
            lv.set_distortion(K, BARREL)
            check(ctx, sc, lv, "plain", K, BARREL, None, mvps, Ms, oracle=False)
            lv.set_distortion(K, np.zeros(5))
            same_as_never()


def test_masked_distorted_level_recovers_the_planted_pose(nmi):
    """The camera frame: the pinhole view of the map from a known pose, seen through a barrel lens (float64 resampler).  With
    distortion set, a masked level's winner is the candidate at that pose (identity warp), scoring strictly higher there than
    the same level without distortion."""
    w, h = 640, 480
    with nmi.NmiContext(w, h) as ctx:
        sc = Scene(nmi, ctx, w, h, False)
        K = lens_K(sc.rp)
        pinhole = sc.frame.cpu().numpy()                  # rendered from camera() + (0.05, 0, 0)
        sc.frame.copy_(dev(unp.distort_image(pinhole, K, BARREL)))
        torch.cuda.synchronize()
        cam = camera()
        offsets = [(0.05 + dx, dy, 0.0) for dx, dy in ((-0.3, 0), (0, 0), (0.3, 0), (0, 0.3), (0, -0.3))]
        mvps = np.stack([capi.render_mvp(sc.rp, *cam, t) for t in offsets])
        Ms = warps(w, h, 9)                               # 3 x 3 x 1: the identity is warp 4
        S, planted = len(offsets), 4 * len(offsets) + 1
        assert np.allclose(Ms[4], np.eye(3))
        with sc.level(S, 9) as lv:
            lv.set_masks(True)
            _, t_plain = (lv.run(mvps, Ms), lv.outputs()[2])
            lv.set_distortion(K, BARREL)
            win, t_dist = check(ctx, sc, lv, "masked", K, BARREL, None, mvps, Ms, oracle=False)
        assert win[0] == planted, (win, planted)
        assert t_dist.reshape(-1)[planted] > t_plain.reshape(-1)[planted], (t_dist.reshape(-1)[planted], t_plain.reshape(-1)[planted])
