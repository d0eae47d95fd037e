"""GPU tests (-m gpu) of masked levels (nmi_level_set_masks / nmi_level_copy_masks) and of the masked pixel-range kernel for
mid-size grids (csrc/nmi_masked_pix_kernel.hip).

The contract: a masked level's replay gives the same renders as before, the same masks as nmi_warp_stack_masked and the same
ratings, winner and score bits as nmi_search_grid_masked on those stacks.  Every comparison is == on bits, computed from the
level's own copied renders, warps and masks: against the standalone calls, against the numpy twin of the masks
(tests/helpers/masked_np.py) and against the oracle's masked search (rounded terms)."""
import os
import subprocess
import time

import numpy as np
import pytest

from helpers import masked_np as mnp
from orbslam2_nmi_amd import capi, sharding, synthetic as sy
from test_render import plane_cloud, plane_mesh

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARP_COUNTS = {1: (1, 1, 1), 3: (3, 1, 1), 8: (2, 2, 2), 9: (3, 3, 1), 12: (3, 2, 2), 27: (3, 3, 3), 81: (9, 9, 1), 243: (9, 9, 3)}


@pytest.fixture(scope="module")
def nmi():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    import orbslam2_nmi_amd as m
    m.load_library()
    return m


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def camera():
    Twc = np.eye(4, dtype=np.float32)
    Twc[:3, 1] = [0, -1, 0]
    return Twc[:3, 3], Twc[:3, 3] + Twc[:3, 2], Twc[:3, 1]


def views(rp, S, scale=1.0):
    """S view matrices around the camera: translations on a small spiral (scale: its size)."""
    cam = camera()
    k = np.arange(S)
    ts = np.stack([0.03 * scale * np.cos(k * 0.9) * (1 + k / 8), 0.03 * scale * np.sin(k * 0.9) * (1 + k / 8), 0.02 * scale * (k % 5 - 2)], -1)
    return np.stack([capi.render_mvp(rp, *cam, tuple(float(v) for v in t)) for t in ts])


def warps(w, h, Wn, scale=1.0):
    return capi.warp_homographies(sy.intrinsics(w, h), WARP_COUNTS[Wn], (0.02 * scale, 0.02 * scale, 0.05 * scale))


def hood_mask(w, h):
    """A hood over the bottom sixth of the frame and a mount in the top-left corner."""
    m = np.ones((h, w), np.uint8)
    m[h - h // 6:] = 0
    m[:h // 8, :w // 10] = 0
    return m


class Scene:
    """Map (point cloud or textured mesh) + the frame a displaced camera sees, on one context."""

    def __init__(self, nmi, ctx, w, h, mesh):
        self.nmi, self.ctx, self.w, self.h = nmi, ctx, w, h
        if mesh:
            xyz, attr, rgb, self.rp = plane_mesh(w, h, nx=12, ny=9)
            self.tex = nmi.NmiTexture(ctx, rgb)
        else:
            xyz, attr, self.rp = plane_cloud(w, h, density=2.0)
            self.tex = None
        self.dx, self.da = dev(xyz), dev(attr)
        view = capi.render_mvp(self.rp, *camera(), (0.05, 0, 0))[None]
        fr = ctx.render_mesh(self.dx, self.da, self.tex, view)[0] if mesh else ctx.render_points(self.dx, torch.sqrt(self.da), view, 3.0)[0]
        self.frame = torch.flip(fr, dims=[0]).contiguous()

    def level(self, S, Wn, block=None):
        return self.nmi.NmiLevel(self.ctx, self.dx, self.da, self.frame, S, Wn, 3.0, texture=self.tex, block=block)


def check(ctx, lv, frame, fm_dev, mvps, Ms, oracle=True):
    """One replay of a masked level against the calls made one after the other.  -> (winner, ratings)"""
    w, h = ctx.width, ctx.height
    win = lv.run(mvps, Ms)
    rs, ws, t = lv.outputs()
    wm, cnt = lv.masks()
    fm = None if fm_dev is None else fm_dev.cpu().numpy()
    assert (wm == mnp.warp_masks((h, w), Ms, fm)).all()
    assert (cnt == np.count_nonzero(wm.reshape(len(Ms), -1), axis=1)).all()
    ws2, wm2 = ctx.warp_stack_masked(frame, Ms, fm_dev)
    assert (ws2.cpu().numpy() == ws).all() and (wm2.cpu().numpy() == wm).all()
    t2 = torch.full(t.shape, -3.0, device="cuda")
    assert ctx.search_grid_masked(dev(rs), dev(ws), dev(wm), t2) == win
    assert (t2.cpu().numpy().view(np.uint32) == t.view(np.uint32)).all()
    if oracle:
        ro, io, bo = mnp.masked_search(rs, ws, wm)
        assert (ro.view(np.uint32) == t.view(np.uint32)).all()
        assert win == (io, bo)
    return win, t


SHAPES = [  # w, h, S, Wn: what scores them
    (160, 120, 27, 27),   # 729 candidates: nmi_masked_grid_kernel
    (160, 128, 9, 9),     # 81: pixel ranges
    (160, 128, 81, 1),
    (160, 128, 1, 81),
    (160, 128, 16, 8),    # 128: pixel ranges
    (160, 128, 4, 8),     # 32: nmi_masked_grid_kernel
    (1241, 376, 3, 3),    # rows not whole 16-byte chunks: the unaligned-row form
    (320, 240, 3, 243),   # many warps, many tables
]


@pytest.mark.parametrize("with_mask", [False, True], ids=["border", "hood"])
@pytest.mark.parametrize("mesh,shape", [(False, s) for s in SHAPES] + [(True, SHAPES[0]), (True, SHAPES[1]), (True, SHAPES[6])],
                         ids=[f"cloud-{s[0]}x{s[1]}-{s[2]}x{s[3]}" for s in SHAPES] + ["mesh-27x27", "mesh-9x9", "mesh-1241x376"])
def test_masked_level_equals_the_calls_one_after_the_other(nmi, mesh, shape, with_mask):
    """Replays with unchanged homographies (the tables are not rebuilt), then changed ones, then changed frame-mask contents."""
    w, h, S, Wn = shape
    with nmi.NmiContext(w, h) as ctx:
        cus = ctx.info()["compute_units"]
        sc = Scene(nmi, ctx, w, h, mesh)
        fm = dev(hood_mask(w, h)) if with_mask else None
        big = S * Wn > 128
        with sc.level(S, Wn) as lv:
            lv.set_masks(True, fm)
            mvps, Ms = views(sc.rp, S), warps(w, h, Wn)
            first = check(ctx, lv, sc.frame, fm, mvps, Ms, oracle=not (big and mesh))
            if cus == 256 and 32 < S * Wn <= 128 and w % 16 == 0:
                assert ctx.pix_status()["last_launch_ranges"] >= 2  # (the standalone search of check(), same routing)
            again = check(ctx, lv, sc.frame, fm, mvps, Ms, oracle=False)  # same warps: same counts, no table rebuilt
            assert again[0] == first[0] and (again[1].view(np.uint32) == first[1].view(np.uint32)).all()
            check(ctx, lv, sc.frame, fm, views(sc.rp, S, 1.7), warps(w, h, Wn, 1.6), oracle=not big)
            if with_mask:
                fm[h // 3:h // 2, w // 3:w // 2] = 0      # the mask's contents change in place: the next replay reads them
                torch.cuda.synchronize()
                check(ctx, lv, sc.frame, fm, mvps, Ms, oracle=not big)
        if w * h <= 320 * 240:
            assert ctx.pix_status()["healed"] == 0  # no helper timed out, no counter wrapped (no bin near 65,536 hits)


def test_levels_and_standalone_searches_interleaved_stay_exact(nmi):
    """Each level owns its counts and tables: two masked levels (different frame masks, hence different counts) and standalone
    masked searches on one context, interleaved; a level whose warps repeat skips its table rebuild and must still be exact."""
    w, h = 160, 128
    with nmi.NmiContext(w, h) as ctx:
        sc = Scene(nmi, ctx, w, h, False)
        fa, fb = dev(hood_mask(w, h)), None
        wl = sy.workload(w, h, 9, 9, seed=5)
        rs, ws = dev(wl["render_stack"]), dev(wl["warp_stack"])
        rng = np.random.default_rng(1)
        other = dev((rng.random((9, h, w)) < 0.7).astype(np.uint8))
        with sc.level(9, 9) as a, sc.level(27, 27) as b:
            a.set_masks(True, fa)
            b.set_masks(True, fb)
            ma, Ma, mb, Mb = views(sc.rp, 9), warps(w, h, 9), views(sc.rp, 27, 0.5), warps(w, h, 27, 0.7)
            ra = check(ctx, a, sc.frame, fa, ma, Ma)
            rb = check(ctx, b, sc.frame, fb, mb, Mb, oracle=False)
            ref = mnp.masked_search(wl["render_stack"], wl["warp_stack"], other.cpu().numpy())  # (the context's bottom-up renders)
            for _ in range(3):
                assert a.run(ma, Ma) == ra[0]
                assert ctx.search_grid_masked(rs, ws, other) == ref[1:]
                assert b.run(mb, Mb) == rb[0]
                t = a.outputs()[2]
                assert (t.view(np.uint32) == ra[1].view(np.uint32)).all()
            check(ctx, a, sc.frame, fa, ma, Ma, oracle=False)
            check(ctx, b, sc.frame, fb, mb, Mb, oracle=False)


def test_off_switch_and_all_ones_frame_mask(nmi):
    w, h, S, Wn = 160, 128, 9, 9
    with nmi.NmiContext(w, h) as ctx:
        sc = Scene(nmi, ctx, w, h, False)
        mvps, Ms = views(sc.rp, S), warps(w, h, Wn)
        with sc.level(S, Wn) as plain, sc.level(S, Wn) as lv:
            ref = plain.run(mvps, Ms)
            t_ref = plain.outputs()[2]
            with pytest.raises(capi.NmiError):
                lv.masks()                                  # no masks yet
            lv.set_masks(True)
            check(ctx, lv, sc.frame, None, mvps, Ms)
            with pytest.raises(ValueError):
                lv.set_masks(False, dev(hood_mask(w, h)))
            assert ctx._lib.nmi_level_set_masks(lv._h, 0, dev(hood_mask(w, h)).data_ptr()) == capi.ERR_INVALID_ARGUMENT
            lv.set_masks(False)                             # the unmasked graph again: the never-masked level's bits
            assert lv.run(mvps, Ms) == ref
            assert (lv.outputs()[2].view(np.uint32) == t_ref.view(np.uint32)).all()
            with pytest.raises(capi.NmiError):
                lv.masks()
        # identity warps have all-ones border masks: an all-ones frame mask then gives the bits of frame_mask=None
        S = 81
        mvps, Ms = views(sc.rp, S), warps(w, h, 1)
        with sc.level(S, 1) as a, sc.level(S, 1) as b:
            a.set_masks(True)
            b.set_masks(True, dev(np.ones((h, w), np.uint8)))
            wa, ta = check(ctx, a, sc.frame, None, mvps, Ms)
            assert a.masks()[0].all()
            wb, tb = check(ctx, b, sc.frame, dev(np.ones((h, w), np.uint8)), mvps, Ms, oracle=False)
            assert wa == wb and (ta.view(np.uint32) == tb.view(np.uint32)).all()


def compose(results):
    """What the MAX all-reduce of the packed keys yields."""
    return capi.key_unpack(max(capi.key_pack(float(s), int(i)) if i >= 0 else 0 for i, s in results))


@pytest.mark.parametrize("mesh", [False, True])
def test_masked_blocks_compose_to_the_masked_level(nmi, mesh):
    """Blocks score their local warps with their own len_w and report global indices; per-block ratings are slices of the
    level's; empty blocks take part in the exchange (RCCL at world size 1)."""
    w, h, S, Wn = 160, 120, 8, 12
    with nmi.NmiContext(w, h) as ctx:
        sc = Scene(nmi, ctx, w, h, mesh)
        fm = dev(hood_mask(w, h))
        mvps, Ms = views(sc.rp, S), warps(w, h, Wn)
        with sc.level(S, Wn) as full:
            full.set_masks(True, fm)
            ref, t_ref = check(ctx, full, sc.frame, fm, mvps, Ms)
            m_ref = full.masks()[0]
            for world in (2, 3):                            # render axis
                got = []
                for rank in range(world):
                    so, sc_, wo, wc = sharding.grid_shard(S, Wn, rank, world)
                    with sc.level(sc_, wc, block=(so, S, wo, Wn)) as blk:
                        blk.set_masks(True, fm)
                        got.append(blk.run(mvps[so:so + sc_], Ms[wo:wo + wc]))
                        _, _, t = blk.outputs()
                        assert (t.view(np.uint32) == t_ref[:, so:so + sc_].view(np.uint32)).all()
                        assert (blk.masks()[0] == m_ref).all()
                assert compose(got) == ref, (world, got, ref)
            got = []                                        # warp axis: the blocks' own len_w
            for wo, wc in ((0, 5), (5, 7)):
                with sc.level(S, wc, block=(0, S, wo, Wn)) as blk:
                    blk.set_masks(True, fm)
                    got.append(blk.run(mvps, Ms[wo:wo + wc]))
                    _, _, t = blk.outputs()
                    m, n = blk.masks()
                    assert (t.view(np.uint32) == t_ref[wo:wo + wc].view(np.uint32)).all()
                    assert (m == m_ref[wo:wo + wc]).all() and (n == np.count_nonzero(m.reshape(wc, -1), axis=1)).all()
            assert compose(got) == ref
            with sc.level(0, Wn, block=(S, S, 0, Wn)) as empty, sc.level(S, Wn, block=(0, S, 0, Wn)) as whole:
                empty.set_masks(True, fm)
                whole.set_masks(True, fm)
                assert empty.run(mvps[:0], Ms) == (-1, np.float32(0))
                comm = ctx.rccl_comm_init(capi.rccl_unique_id(), 0, 1)
                try:
                    assert empty.run_rccl(mvps[:0], Ms, comm) == (-1, np.float32(0))
                    assert whole.run_rccl(mvps, Ms, comm) == ref
                    assert (whole.outputs()[2].view(np.uint32) == t_ref.view(np.uint32)).all()
                finally:
                    capi.rccl_comm_destroy(comm)


@pytest.mark.parametrize("S,Wn", [(9, 9), (27, 27)], ids=["pixel-ranges", "grid-kernel"])
def test_counter_wraps_in_masked_levels(nmi, S, Wn):
    """A flat frame and a one-colour cloud at 640x480: at most four joint bins share ~290,000 masked pixels, so some bin holds
    more than 65,535 hits and a 16-bit counter wraps (in a helper, an owner or the merge, or in a grid workgroup)."""
    w, h = 640, 480
    xyz, red, rp = plane_cloud(w, h, density=1.2)
    with nmi.NmiContext(w, h) as ctx:
        dx, dr = dev(xyz), dev(np.full_like(red, 0.5))
        frame = dev(np.full((h, w), 100, np.uint8))
        fm = np.ones((h, w), np.uint8)
        fm[h - 20:] = 0
        fm = dev(fm)
        with nmi.NmiLevel(ctx, dx, dr, frame, S, Wn, 3.0) as lv:
            lv.set_masks(True, fm)
            mvps, Ms = views(rp, S), warps(w, h, Wn)
            check(ctx, lv, frame, fm, mvps, Ms, oracle=S * Wn <= 81)
            rs, ws, _ = lv.outputs()
            wm, _ = lv.masks()
            j, _, _ = mnp.masked_hist(rs[0], ws[0], wm[0])
            assert j.max() > 65535  # (the premise)


def wrap_stacks(w, h):
    yy, xx = np.mgrid[0:h, 0:w]
    a = np.where((xx + yy) % 2 == 0, 10, 200).astype(np.uint8)
    b = np.where((xx // 2 + yy) % 2 == 0, 30, 90).astype(np.uint8)
    c = np.where(xx % 7 == 0, 30, 90).astype(np.uint8)
    rs = np.stack([a, np.where(xx % 3 == 0, 10, 200).astype(np.uint8)] * 16)[:32]
    return rs, np.stack([b, c])


def test_counter_wraps_in_the_masked_pixel_range_kernel(nmi):
    """test_pix_kernel's wrap pattern under masks that keep most pixels: bins of ~70,000 hits wrap in helpers, owners and merges;
    the count test (decoded total != pixels added by all ranges) sends those candidates to the masked exact path."""
    w, h = 640, 480
    rs, ws = wrap_stacks(w, h)
    masks = np.ones((2, h, w), np.uint8)
    masks[0, h - 30:] = 0
    masks[1, :, :11] = 0
    ro, io, bo = mnp.masked_search(rs, ws, masks, render_bottom_up=False)
    for ranges in (2, 3, 4):
        with nmi.NmiContext(w, h, render_bottom_up=False) as ctx:
            ctx.set_option(ctx.OPT_SPLIT, 1)
            ctx.set_option(ctx.OPT_SPLIT_PIXELS, ranges)
            t = torch.zeros((2, 32), device="cuda")
            got = ctx.search_grid_masked(dev(rs), dev(ws), dev(masks), t)
            assert ctx.pix_status()["last_launch_ranges"] == ranges
        assert got == (io, bo), ranges
        assert (t.cpu().numpy().view(np.uint32) == ro.view(np.uint32)).all(), ranges


@pytest.mark.parametrize("S,Wn,w,h", [(9, 9, 160, 128), (11, 3, 160, 128), (1, 128, 160, 128), (85, 1, 176, 96), (16, 8, 160, 128),
                                      (6, 6, 1241, 376)])
def test_standalone_mid_size_masked_search(nmi, S, Wn, w, h):
    """nmi_search_grid_masked at 33 ... 128 candidates (and an unaligned-row frame) takes pixel ranges and equals the oracle."""
    wl = sy.workload(w, h, S, Wn, seed=S * 7 + Wn)
    rng = np.random.default_rng(S + Wn)
    masks = (rng.random((Wn, h, w)) < 0.8).astype(np.uint8)
    masks[:, h - h // 5:] = 0
    ro, io, bo = mnp.masked_search(wl["render_stack"], wl["warp_stack"], masks, render_bottom_up=wl["bottom_up"])
    with nmi.NmiContext(w, h, render_bottom_up=wl["bottom_up"]) as ctx:
        cus = ctx.info()["compute_units"]
        t = torch.full((Wn, S), -3.0, device="cuda")
        got = ctx.search_grid_masked(dev(wl["render_stack"]), dev(wl["warp_stack"]), dev(masks), t)
        st = ctx.pix_status()
    if cus == 256:
        assert st["last_launch_ranges"] >= 2, st
    assert st["healed"] == 0
    assert got == (io, bo)
    assert (t.cpu().numpy().view(np.uint32) == ro.view(np.uint32)).all()


def test_a_missing_helper_is_healed_inside_the_launch(nmi):
    """Phase-mask bit 9 (test hook): helper 1 of every candidate withholds its flags, so every owner gives up after its bounded
    wait and scores the candidate alone on the masked exact path -- inside the one launch, with the oracle's bits."""
    w, h, S, Wn = 160, 128, 9, 5
    wl = sy.workload(w, h, S, Wn, seed=3)
    rng = np.random.default_rng(4)
    masks = (rng.random((Wn, h, w)) < 0.6).astype(np.uint8)
    ro, io, bo = mnp.masked_search(wl["render_stack"], wl["warp_stack"], masks, render_bottom_up=wl["bottom_up"])
    rs, ws, wm = dev(wl["render_stack"]), dev(wl["warp_stack"]), dev(masks)
    with nmi.NmiContext(w, h, render_bottom_up=wl["bottom_up"]) as ctx:
        ctx.set_option(ctx.OPT_SPLIT, 1)
        ctx.set_option(ctx.OPT_SPLIT_PIXELS, 3)
        assert ctx.search_grid_masked(rs, ws, wm) == (io, bo)
        assert ctx.pix_status() == {"last_launch_ranges": 3, "healed": 0}
        ctx.set_option(ctx.OPT_PHASE_MASK, 3 | 512)
        t = torch.zeros((Wn, S), device="cuda")
        t0 = time.perf_counter()
        assert ctx.search_grid_masked(rs, ws, wm, t) == (io, bo)
        assert time.perf_counter() - t0 < 0.5
        assert (t.cpu().numpy().view(np.uint32) == ro.view(np.uint32)).all()
        assert ctx.pix_status() == {"last_launch_ranges": 3, "healed": S * Wn}
        ctx.set_option(ctx.OPT_PHASE_MASK, 3)
        assert ctx.search_grid_masked(rs, ws, wm) == (io, bo)     # the stale blocks of that launch carry an old tag
        assert ctx.pix_status()["healed"] == S * Wn


def test_level_pipeline_masked_recovers_planted_offset():
    exe = os.path.join(ROOT, "examples", "level_pipeline")
    if not os.access(exe, os.X_OK):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples")], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    r = subprocess.run([exe, "20", "--masked"], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "masked levels:" in r.stdout and "PIPELINE OK" in r.stdout
