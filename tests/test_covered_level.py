"""GPU tests (-m gpu) of covered levels (nmi_level_set_coverage / nmi_level_copy_coverage).

The contract: a covered level's replay gives the same renders as the unmasked level, the same coverage masks as
nmi_render_*_masked, the same warp masks as nmi_warp_stack_masked, and the same ratings, winner, score bits and len[w][s] as
nmi_search_grid_covered on those stacks.  Every comparison is == on bits: against the standalone chain, against the numpy twin
of the warp masks (tests/helpers/masked_np.py) and, at small sizes, against the covered numpy model (tests/helpers/covered_np.py,
oracle terms rounded)."""
import os
import subprocess

import numpy as np
import pytest

from helpers import covered_np as cnp
from helpers import masked_np as mnp
from orbslam2_nmi_amd import capi, sharding, synthetic as sy
from test_masked_level import SHAPES, Scene, compose, dev, hood_mask, views, warps

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def nmi():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    import orbslam2_nmi_amd as m
    m.load_library()
    return m


class CoveredScene(Scene):
    """Scene whose map has a hole: the frame is rendered from the whole map, the levels and the chain from the map without the
    points / triangles that project into a rectangle of the reference view, so part of every render keeps the clear colour."""

    def __init__(self, nmi, ctx, w, h, mesh):
        super().__init__(nmi, ctx, w, h, mesh)
        xyz, attr = self.dx.cpu().numpy(), self.da.cpu().numpy()
        per = 3 if mesh else 1
        first = xyz.reshape(-1, per, 3)[:, 0]
        u = first[:, 0] / first[:, 2] * self.rp.fx + self.rp.cx
        v = first[:, 1] / first[:, 2] * self.rp.fy + self.rp.cy
        keep = ~((u >= 0.3 * w) & (u < 0.6 * w) & (v >= 0.25 * h) & (v < 0.65 * h))
        self.dx = dev(xyz.reshape(-1, per, 3)[keep].reshape(-1, 3))
        self.da = dev(attr.reshape((-1, per) + attr.shape[1:])[keep].reshape((-1,) + attr.shape[1:]))
        self.mesh = mesh

    def chain_renders(self, ctx, mvps):
        if self.mesh:
            return ctx.render_mesh_masked(self.dx, self.da, self.tex, mvps)
        return ctx.render_points_masked(self.dx, self.da, mvps, 3.0)


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def check(ctx, sc, lv, fm_dev, mvps, Ms, oracle=True, plain=None):
    """One replay of a covered level against the chain nmi_render_*_masked -> nmi_warp_stack_masked -> nmi_search_grid_covered.
    plain: an unmasked level of the same map, whose renders must be the covered level's.  -> (winner, ratings)"""
    w, h = ctx.width, ctx.height
    win = lv.run(mvps, Ms)
    rs, ws, t = lv.outputs()
    rm, wm, cnt = lv.coverage()
    fm = None if fm_dev is None else fm_dev.cpu().numpy()
    assert (wm == mnp.warp_masks((h, w), Ms, fm)).all()
    rs2, rm2 = sc.chain_renders(ctx, mvps)
    assert (rs2.cpu().numpy() == rs).all() and (rm2.cpu().numpy() == rm).all()
    ws2, wm2 = ctx.warp_stack_masked(sc.frame, Ms, fm_dev)
    assert (ws2.cpu().numpy() == ws).all() and (wm2.cpu().numpy() == wm).all()
    t2 = torch.full(t.shape, -3.0, device="cuda")
    assert ctx.search_grid_covered(rs2, rm2, ws2, wm2, t2) == win
    assert (bits(t2.cpu().numpy()) == bits(t)).all()
    assert (ctx.cover_counts(t.size).reshape(t.shape) == cnt).all()
    assert (cnt == cnp.cover_counts(wm, rm)).all()
    if plain is not None:
        plain.run(mvps, Ms)
        assert (plain.outputs()[0] == rs).all()
    if oracle:
        ro, io, bo, _ = cnp.covered_search(rs, ws, wm, rm)
        assert (bits(ro) == bits(t)).all()
        assert win == (io, bo)
    return win, t


@pytest.mark.parametrize("with_mask", [False, True], ids=["border", "hood"])
@pytest.mark.parametrize("mesh,shape", [(False, s) for s in SHAPES] + [(True, SHAPES[0]), (True, SHAPES[1]), (True, SHAPES[6])],
                         ids=[f"cloud-{s[0]}x{s[1]}-{s[2]}x{s[3]}" for s in SHAPES] + ["mesh-27x27", "mesh-9x9", "mesh-1241x376"])
def test_covered_level_equals_the_chain(nmi, mesh, shape, with_mask):
    """Replays with unchanged parameters, then changed views and warps, then changed frame-mask contents.  The point-cloud
    shapes take the fused front (double-buffered anchors, the epoch-aware coverage resolve) except 1241x376, whose frame rows are
    not 16-byte aligned (the unfused render)."""
    w, h, S, Wn = shape
    with nmi.NmiContext(w, h) as ctx:
        cus = ctx.info()["compute_units"]
        sc = CoveredScene(nmi, ctx, w, h, mesh)
        fm = dev(hood_mask(w, h)) if with_mask else None
        big = S * Wn > 128
        with sc.level(S, Wn) as lv, sc.level(S, Wn) as plain:
            lv.set_coverage(True, fm)
            mvps, Ms = views(sc.rp, S), warps(w, h, Wn)
            first = check(ctx, sc, lv, fm, mvps, Ms, oracle=not (big and mesh), plain=plain)
            if cus == 256 and 32 < S * Wn <= 128 and w % 16 == 0:
                assert ctx.pix_status()["last_launch_ranges"] >= 2  # (the chain's search, same routing as the level's)
            rm = lv.coverage()[0]
            assert 0 < np.count_nonzero(rm) < rm.size  # (the premise: the map leaves part of the view uncovered)
            again = check(ctx, sc, lv, fm, mvps, Ms, oracle=False)
            assert again[0] == first[0] and (bits(again[1]) == bits(first[1])).all()
            check(ctx, sc, lv, fm, views(sc.rp, S, 1.7), warps(w, h, Wn, 1.6), oracle=not big, plain=plain)
            if with_mask:
                fm[h // 3:h // 2, w // 3:w // 2] = 0      # the mask's contents change in place: the next replay reads them
                torch.cuda.synchronize()
                check(ctx, sc, lv, fm, mvps, Ms, oracle=not big)
        if w * h <= 320 * 240:
            assert ctx.pix_status()["healed"] == 0


def test_covered_levels_and_standalone_searches_interleaved_stay_exact(nmi):
    """Each level owns its masks, counts and redo list: two covered levels (one mid-size, one 729-candidate) and standalone
    covered searches of other sizes on one context, interleaved."""
    w, h = 160, 128
    with nmi.NmiContext(w, h) as ctx:
        sc = CoveredScene(nmi, ctx, w, h, False)
        fa = dev(hood_mask(w, h))
        wl = sy.workload(w, h, 9, 9, seed=5)
        rs, ws = dev(wl["render_stack"]), dev(wl["warp_stack"])
        rng = np.random.default_rng(1)
        wm_o = (rng.random((9, h, w)) < 0.7).astype(np.uint8)
        rm_o = (rng.random((9, h, w)) < 0.8).astype(np.uint8)
        ref = cnp.covered_search(wl["render_stack"], wl["warp_stack"], wm_o, rm_o)
        with sc.level(9, 9) as a, sc.level(27, 27) as b:
            a.set_coverage(True, fa)
            b.set_coverage(True)
            ma, Ma, mb, Mb = views(sc.rp, 9), warps(w, h, 9), views(sc.rp, 27, 0.5), warps(w, h, 27, 0.7)
            ra = check(ctx, sc, a, fa, ma, Ma)
            rb = check(ctx, sc, b, None, mb, Mb, oracle=False)
            ca, cb = a.coverage()[2], b.coverage()[2]
            for _ in range(3):
                assert a.run(ma, Ma) == ra[0]
                assert ctx.search_grid_covered(rs, dev(rm_o), ws, dev(wm_o)) == ref[1:3]
                assert (ctx.cover_counts(81).reshape(9, 9) == ref[3]).all()
                assert b.run(mb, Mb) == rb[0]
                assert (bits(a.outputs()[2]) == bits(ra[1])).all() and (a.coverage()[2] == ca).all()
                assert (bits(b.outputs()[2]) == bits(rb[1])).all() and (b.coverage()[2] == cb).all()
            check(ctx, sc, a, fa, ma, Ma, oracle=False)
            check(ctx, sc, b, None, mb, Mb, oracle=False)


def test_coverage_off_switch_and_mode_rules(nmi):
    w, h, S, Wn = 160, 128, 9, 9
    with nmi.NmiContext(w, h) as ctx:
        sc = CoveredScene(nmi, ctx, w, h, False)
        mvps, Ms = views(sc.rp, S), warps(w, h, Wn)
        fm = dev(hood_mask(w, h))
        lib = ctx._lib
        with sc.level(S, Wn) as plain, sc.level(S, Wn) as lv, sc.level(S, Wn) as masked:
            ref = plain.run(mvps, Ms)
            t_ref = plain.outputs()[2]
            with pytest.raises(capi.NmiError):
                lv.coverage()                               # no coverage yet
            lv.set_coverage(True, fm)
            win, t = check(ctx, sc, lv, fm, mvps, Ms)
            with pytest.raises(ValueError):
                lv.set_coverage(False, fm)
            assert lib.nmi_level_set_coverage(lv._h, 0, fm.data_ptr()) == capi.ERR_INVALID_ARGUMENT
            assert lib.nmi_level_set_coverage(lv._h, 2, None) == capi.ERR_INVALID_ARGUMENT
            # covered -> masked is refused and leaves the covered level as it was
            assert lib.nmi_level_set_masks(lv._h, 1, None) == capi.ERR_INVALID_ARGUMENT
            assert lib.nmi_level_set_masks(lv._h, 1, fm.data_ptr()) == capi.ERR_INVALID_ARGUMENT
            with pytest.raises(capi.NmiError):
                lv.masks()                                  # nmi_level_copy_masks: not a masked level
            assert lv.run(mvps, Ms) == win and (bits(lv.outputs()[2]) == bits(t)).all()
            check(ctx, sc, lv, fm, mvps, Ms, oracle=False)
            # masked -> covered is refused and leaves the masked level as it was
            masked.set_masks(True, fm)
            mw = masked.run(mvps, Ms)
            mt = masked.outputs()[2]
            assert lib.nmi_level_set_coverage(masked._h, 1, None) == capi.ERR_INVALID_ARGUMENT
            assert lib.nmi_level_set_coverage(masked._h, 1, fm.data_ptr()) == capi.ERR_INVALID_ARGUMENT
            with pytest.raises(capi.NmiError):
                masked.coverage()
            assert masked.run(mvps, Ms) == mw and (bits(masked.outputs()[2]) == bits(mt)).all()
            masked.masks()
            # off: the unmasked graph again, the never-covered level's bits
            lv.set_coverage(False)
            assert lv.run(mvps, Ms) == ref
            assert (bits(lv.outputs()[2]) == bits(t_ref)).all()
            with pytest.raises(capi.NmiError):
                lv.coverage()
            # and on again, now with border masks only
            lv.set_coverage(True)
            check(ctx, sc, lv, None, mvps, Ms)


@pytest.mark.parametrize("mesh", [False, True])
def test_covered_blocks_compose_to_the_covered_level(nmi, mesh):
    """Blocks score their local candidates with their own len[w][s] and report global indices; per-block ratings and counts are
    slices of the level's; empty blocks take part in the exchange (RCCL at world size 1)."""
    w, h, S, Wn = 160, 120, 8, 12
    with nmi.NmiContext(w, h) as ctx:
        sc = CoveredScene(nmi, ctx, w, h, mesh)
        fm = dev(hood_mask(w, h))
        mvps, Ms = views(sc.rp, S), warps(w, h, Wn)
        with sc.level(S, Wn) as full:
            full.set_coverage(True, fm)
            ref, t_ref = check(ctx, sc, full, fm, mvps, Ms)
            r_ref, m_ref, c_ref = full.coverage()
            for world in (2, 3):                            # render axis
                got = []
                for rank in range(world):
                    so, sc_, wo, wc = sharding.grid_shard(S, Wn, rank, world)
                    with sc.level(sc_, wc, block=(so, S, wo, Wn)) as blk:
                        blk.set_coverage(True, fm)
                        got.append(blk.run(mvps[so:so + sc_], Ms[wo:wo + wc]))
                        t = blk.outputs()[2]
                        r, m, c = blk.coverage()
                        assert (bits(t) == bits(t_ref[:, so:so + sc_])).all()
                        assert (r == r_ref[so:so + sc_]).all() and (m == m_ref).all() and (c == c_ref[:, so:so + sc_]).all()
                assert compose(got) == ref, (world, got, ref)
            got = []                                        # warp axis
            for wo, wc in ((0, 5), (5, 7)):
                with sc.level(S, wc, block=(0, S, wo, Wn)) as blk:
                    blk.set_coverage(True, fm)
                    got.append(blk.run(mvps, Ms[wo:wo + wc]))
                    t = blk.outputs()[2]
                    r, m, c = blk.coverage()
                    assert (bits(t) == bits(t_ref[wo:wo + wc])).all()
                    assert (m == m_ref[wo:wo + wc]).all() and (c == c_ref[wo:wo + wc]).all()
            assert compose(got) == ref
            with sc.level(0, Wn, block=(S, S, 0, Wn)) as empty, sc.level(S, Wn, block=(0, S, 0, Wn)) as whole:
                empty.set_coverage(True, fm)
                whole.set_coverage(True, fm)
                empty.coverage()                            # nothing was produced: nothing to copy
                assert empty.run(mvps[:0], Ms) == (-1, np.float32(0))
                comm = ctx.rccl_comm_init(capi.rccl_unique_id(), 0, 1)
                try:
                    assert empty.run_rccl(mvps[:0], Ms, comm) == (-1, np.float32(0))
                    assert whole.run_rccl(mvps, Ms, comm) == ref
                    assert (bits(whole.outputs()[2]) == bits(t_ref)).all()
                finally:
                    capi.rccl_comm_destroy(comm)


@pytest.mark.parametrize("S,Wn", [(9, 9), (27, 27)], ids=["pixel-ranges", "grid-kernel"])
def test_counter_wraps_in_covered_levels(nmi, S, Wn):
    """A flat frame and a one-colour cloud at 640x480: at most four joint bins share ~250,000 covered pixels, so some bin holds
    more than 65,535 hits and a 16-bit counter wraps (in a helper, an owner or the merge, or in a grid workgroup)."""
    from test_render import plane_cloud
    w, h = 640, 480
    xyz, red, rp = plane_cloud(w, h, density=1.2)
    u = xyz[:, 0] / xyz[:, 2] * rp.fx + rp.cx
    keep = ~((u >= 0.4 * w) & (u < 0.5 * w))                # a band of the view the map does not cover
    with nmi.NmiContext(w, h) as ctx:
        dx, dr = dev(xyz[keep]), dev(np.full_like(red[keep], 0.5))
        frame = dev(np.full((h, w), 100, np.uint8))
        fm = np.ones((h, w), np.uint8)
        fm[h - 20:] = 0
        fm = dev(fm)

        class Flat:
            mesh, tex = False, None

            def chain_renders(self, c, mvps):
                return c.render_points_masked(dx, dr, mvps, 3.0)
        sc = Flat()
        sc.frame = frame
        with nmi.NmiLevel(ctx, dx, dr, frame, S, Wn, 3.0) as lv:
            lv.set_coverage(True, fm)
            mvps, Ms = views(rp, S), warps(w, h, Wn)
            check(ctx, sc, lv, fm, mvps, Ms, oracle=S * Wn <= 81)
            rs, ws, _ = lv.outputs()
            rm, wm, cnt = lv.coverage()
            assert cnt.min() < w * h - 20 * w  # (the premise: coverage removes pixels)
            j, _, _ = mnp.masked_hist(rs[0], ws[0], cnp.pair_mask(wm[0], rm[0]).astype(np.uint8))
            assert j.max() > 65535  # (the premise: a counter wraps)


@pytest.mark.parametrize("args", [["20", "--covered"], ["20", "--mesh", "--covered"]], ids=["cloud", "mesh"])
def test_level_pipeline_covered_recovers_planted_offset(args):
    exe = os.path.join(ROOT, "examples", "level_pipeline")
    if not os.access(exe, os.X_OK):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples")], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "covered levels:" in r.stdout and "PIPELINE OK" in r.stdout
