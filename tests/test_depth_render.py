"""Depth renders (include/nmi_hip.h, "Depth maps"), GPU tier: nmi_depth_shade_apply over all 2^24 depths, nmi_render_points_depth
and nmi_render_mesh_depth on the hard clouds and meshes of tests/helpers/render_cases.py and mesh_cases.py, the closed loop with
the deep-frame intake, and the argument errors.  `==` on every byte, against the twin of tests/helpers/depth_np.py applied to the
depths the committed oracles expose (no rasteriser of its own here).  The CPU tier is tests/test_depth_shade.py.
"""
import ctypes as C
import time

import numpy as np
import pytest

from helpers import depth_np as dn
from helpers import mesh_cases as mc
from helpers import mesh_color as col
from helpers import render_cases as rc

try:
    import torch
except ImportError:  # the CPU tier does not need it
    torch = None

f32 = np.float32
# The cases' projections are rc.ZN = 5, rc.ZF = 30.  SHADES[0]: millimetres, 5000 .. 30000, a window inside the range so that both
# of its ends are reached; SHADES[1]: 2500 units per metre, 12500 .. 75000: the far part clamps at 65535, the window's hi above it.
SHADES = [dn.make(rc.ZN, rc.ZF, 1000.0, 6000, 28000), dn.make(rc.ZN, rc.ZF, 2500.0, 0, 65535)]
POINT_SHAPES = [(160, 120), (150, 90), (40, 30), (130, 129)]     # fast strips (width % 4 == 0) and the any-size kernel
POINT_SIZES = [1, 2, 5, 6]                                       # fast strips take sizes <= 5
HEAVY = {"full_bins", "frustum_margin", "far_from_origin", "tessellation", "depth"}     # test_mesh_edges.HEAVY
MESH_SIZES = [(160, 120), (150, 90), (40, 30), (130, 129)]                               # test_mesh_edges.GPU_SIZES
MESH_CASES = [(f, s) for f in mc.EXPECTED_BRANCHES for s in MESH_SIZES if f not in HEAVY or s == (150, 90)]


def test_constants_are_the_mesh_tests():
    import test_mesh_edges as te
    assert (HEAVY, MESH_SIZES) == (te.HEAVY, te.GPU_SIZES)


@pytest.fixture(scope="module")
def nmi():
    if torch is None or not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    import orbslam2_nmi_amd as m
    m.load_library()
    return m


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def cshade(sh):
    from orbslam2_nmi_amd import capi
    return capi.NmiDepthShade(**sh)


def u16(t):
    return t.cpu().numpy().view(np.uint16)


def differs(tag, got, want):
    """(grey, v, mask) stacks, got against want -> list of complaints."""
    bad = []
    for name, g, w in zip(("grey", "depth16", "mask"), got, want):
        for s in range(len(w)):
            d = g[s] != w[s]
            if d.any():
                yy, xx = np.nonzero(d)
                bad.append(f"{tag} {name} view {s}: {int(d.sum())} px differ, first ({xx[0]}, {yy[0]}): got {g[s][yy[0], xx[0]]} twin {w[s][yy[0], xx[0]]}")
    return bad


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(len(SHADES)))
def test_gpu_depth_shade_apply_all_depths(nmi, k):
    """All 2^24 depths in one call: v and grey equal the twin's."""
    sh = SHADES[k]
    d = np.arange(1 << 24, dtype=np.int32)
    want_v, want_g = dn.shade(d, sh)
    with nmi.NmiContext(64, 48) as ctx:
        v, g = ctx.depth_shade_apply(cshade(sh), dev(d))
        v, g = u16(v), g.cpu().numpy()
    assert want_v.min() >= 1
    if k == 0:
        assert len(np.unique(want_g)) == 256                                  # every grey of the window
    if k == 1:
        assert want_v.max() == 65535 and (want_v == 65535).sum() > 1000      # the clamp is reached
    nv, ng = int((v != want_v).sum()), int((g != want_g).sum())
    assert nv == 0 and ng == 0, f"{nv} raw depths and {ng} greys of 2^24 differ; first at d = {int(np.argmax((v != want_v) | (g != want_g)))}"


@pytest.mark.gpu
@pytest.mark.parametrize("size", POINT_SIZES)
@pytest.mark.parametrize("shape", POINT_SHAPES, ids=[f"{w}x{h}" for w, h in POINT_SHAPES])
def test_gpu_render_points_depth_families(nmi, shape, size):
    """Every family of render_cases at this frame and point size, with the cloud's reds and without any: grey, depth16 and mask
    equal the twin's; with reds the mask is nmi_render_points_masked's byte for byte.  Both shades in turn over the cases."""
    W, H = shape
    bad, covered = [], 0
    with nmi.NmiContext(W, H) as ctx:
        n = 0
        for family, cases in rc.families(W, H).items():
            for i, c in enumerate(cases):
                sh = SHADES[n % 2]
                n += 1
                dx, dr = dev(c["xyz"]), dev(c["red"])
                _, colour_mask = ctx.render_points_masked(dx, dr, c["mvps"], size)
                for red, dred in ((c["red"], dr), (None, None)):
                    tag = f"{family}[{i}] size {size} {'with' if red is not None else 'no'} red"
                    want = dn.points_stack(c["xyz"], red, c["mvps"], W, H, size, sh)
                    g, m, v = ctx.render_points_depth(dx, dred, c["mvps"], size, cshade(sh), out_masks=True, depth16=True)
                    bad += differs(tag, (g.cpu().numpy(), u16(v), m.cpu().numpy()), want)
                    covered += int(want[2].sum())
                    if red is not None and not torch.equal(m, colour_mask):
                        bad.append(f"{tag}: the mask differs from nmi_render_points_masked's")
                    # the outputs are optional one by one: the grey alone is the same grey
                    g1, m1, v1 = ctx.render_points_depth(dx, dred, c["mvps"], size, cshade(sh))
                    if m1 is not None or v1 is not None or not torch.equal(g1, g):
                        bad.append(f"{tag}: the render without masks and depth16 differs")
    assert covered > 0
    assert not bad, bad[:10]


@pytest.mark.gpu
def test_gpu_points_depth_unaligned_depth16(nmi):
    """A depth16 stack that is only 2-byte aligned takes the any-size kernel's stores: the same bytes."""
    W, H, size = 160, 120, 3
    c = rc.families(W, H)["edges"][0]
    sh = SHADES[0]
    want = dn.points_stack(c["xyz"], c["red"], c["mvps"], W, H, size, sh)
    S = len(c["mvps"])
    with nmi.NmiContext(W, H) as ctx:
        buf = torch.zeros(S * H * W + 1, dtype=torch.int16, device="cuda")
        v = buf[1:].view(S, H, W)
        assert v.data_ptr() % 8 == 2
        g, m, _ = ctx.render_points_depth(dev(c["xyz"]), dev(c["red"]), c["mvps"], size, cshade(sh), out_masks=True, depth16=v)
        assert not differs("unaligned", (g.cpu().numpy(), u16(v), m.cpu().numpy()), want)
        assert int(buf[0]) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("family,shape", MESH_CASES, ids=[f"{s[0]}x{s[1]}-{f}" for f, s in MESH_CASES])
def test_gpu_render_mesh_depth_families(nmi, family, shape):
    """nmi_render_mesh_depth against the twin (grey, depth16, mask); the mask equals nmi_render_mesh_colored_masked's on the same
    mesh; one image whatever the tile queue's and the clip queue's capacity (LDS records, memory-buffer path, bin overflow)."""
    W, H = shape
    bad, covered = [], 0
    t0 = time.time()
    with nmi.NmiContext(W, H) as ctx:
        for i, c in enumerate(mc.family(family, W, H)):
            tag = f"{family}[{i}]"
            sh = SHADES[i % 2]
            want = dn.mesh_stack(col.twin_of(family, W, H, i), sh)
            covered += int(want[2].sum())
            dx = dev(c["xyz"])
            g, m, v = ctx.render_mesh_depth(dx, c["mvps"], cshade(sh), out_masks=True, depth16=True)
            bad += differs(tag, (g.cpu().numpy(), u16(v), m.cpu().numpy()), want)
            _, colour_mask = ctx.render_mesh_colored_masked(dx, dev(col.colors_of(family, W, H, i)), c["mvps"])
            if not torch.equal(m, colour_mask):
                bad.append(f"{tag}: the mask differs from nmi_render_mesh_colored_masked's")
            g1, m1, v1 = ctx.render_mesh_depth(dx, c["mvps"], cshade(sh))
            if m1 is not None or v1 is not None or not torch.equal(g1, g):
                bad.append(f"{tag}: the render without masks and depth16 differs")
            for cap, clip_cap in ((5, 1 << 18), (0, 1 << 18), (4 << 20, 2)):
                ctx.set_option(ctx.OPT_TILE_QUEUE, cap)
                ctx.set_option(ctx.OPT_CLIP_QUEUE, clip_cap)
                g2, m2, v2 = ctx.render_mesh_depth(dx, c["mvps"], cshade(sh), out_masks=True, depth16=True)
                if not (torch.equal(g2, g) and torch.equal(m2, m) and torch.equal(v2, v)):
                    bad.append(f"{tag}: tile queue {cap} / clip queue {clip_cap} gives another image")
            ctx.set_option(ctx.OPT_TILE_QUEUE, 4 << 20)
            ctx.set_option(ctx.OPT_CLIP_QUEUE, 1 << 18)
    print(f"{family} {W}x{H}: {covered} covered pixels, {time.time() - t0:.1f} s")
    assert not bad, bad[:10]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["points", "mesh"])
def test_gpu_closed_loop_with_the_intake(nmi, kind):
    """d_depth16 of a view, fed as a GRAY16 frame through nmi_deep_frame under NMI_TONE_WINDOW(lo, hi), 16 bits, valid range
    (1, 65535): the grey equals the render's grey on covered pixels, the validity mask equals the coverage mask everywhere."""
    from orbslam2_nmi_amd import capi
    W, H = 160, 120
    sh = SHADES[0]
    with nmi.NmiContext(W, H) as ctx:
        if kind == "points":
            c = rc.families(W, H)["edges"][0]
            g, m, v = ctx.render_points_depth(dev(c["xyz"]), None, c["mvps"], 5, cshade(sh), out_masks=True, depth16=True)
        else:
            c = mc.family("tessellation", W, H)[0]
            g, m, v = ctx.render_mesh_depth(dev(c["xyz"]), c["mvps"], cshade(sh), out_masks=True, depth16=True)
        ctx.set_tone_map(capi.ToneMap.window(sh["lo"], sh["hi"], bits=16))
        ctx.set_valid_range(1, 65535)
        n = 0
        for s in range(len(c["mvps"])):
            src = v[s].contiguous().view(torch.uint8)
            grey, valid = ctx.deep_frame(src)
            cov = m[s] != 0
            n += int(cov.sum())
            assert torch.equal(valid, m[s]), f"view {s}: validity and coverage differ on {int((valid != m[s]).sum())} pixels"
            assert torch.equal(grey[cov], g[s][cov]), f"view {s}: the intake's grey differs from the render's on covered pixels"
        assert n > 0


@pytest.mark.gpu
def test_gpu_depth_argument_errors(nmi):
    """Each bad argument is refused with nothing launched (the outputs keep their bytes), and the next valid call is correct."""
    from orbslam2_nmi_amd import capi
    from test_depth_shade import bad_shades
    W, H = 40, 30
    c = mc.family("tessellation", W, H)[0]
    p = rc.families(W, H)["edges"][0]
    T = len(c["xyz"]) // 3
    sh = SHADES[0]
    want_mesh = dn.mesh_stack(col.twin_of("tessellation", W, H, 0), sh)
    want_pts = dn.points_stack(p["xyz"], None, p["mvps"][:1], W, H, 2, sh)
    E = capi.ERR_INVALID_ARGUMENT
    good, bad = bad_shades()
    with nmi.NmiContext(W, H) as ctx:
        lib, h = ctx._lib, ctx._h
        dx, dp = dev(c["xyz"]), dev(p["xyz"])
        out = torch.full((1, H, W), 7, dtype=torch.uint8, device="cuda")
        msk = torch.full((1, H, W), 7, dtype=torch.uint8, device="cuda")
        d16 = torch.full((1, H, W), 7, dtype=torch.int16, device="cuda")
        d24 = torch.zeros(16, dtype=torch.int32, device="cuda")
        m = np.ascontiguousarray(c["mvps"][:1], f32)
        mp = m.ctypes.data_as(C.POINTER(C.c_float))
        torch.cuda.synchronize()
        g = C.byref(good)

        def check_after(tag):
            ctx.synchronize()
            torch.cuda.synchronize()
            assert (out == 7).all() and (msk == 7).all() and (d16 == 7).all(), tag
            got = ctx.render_mesh_depth(dx, c["mvps"], cshade(sh), out_masks=True, depth16=True)
            assert not differs(tag + ": mesh after", (got[0].cpu().numpy(), u16(got[2]), got[1].cpu().numpy()), want_mesh)
            got = ctx.render_points_depth(dp, None, p["mvps"][:1], 2, cshade(sh), out_masks=True, depth16=True)
            assert not differs(tag + ": points after", (got[0].cpu().numpy(), u16(got[2]), got[1].cpu().numpy()), want_pts)

        for i, s in enumerate([None] + bad):
            ref = C.byref(s) if s is not None else None
            assert lib.nmi_render_points_depth(h, dp.data_ptr(), None, len(p["xyz"]), mp, 1, 2.0, ref, out.data_ptr(), msk.data_ptr(), d16.data_ptr()) == E
            assert lib.nmi_render_mesh_depth(h, dx.data_ptr(), T, mp, 1, ref, out.data_ptr(), msk.data_ptr(), d16.data_ptr()) == E
            assert lib.nmi_depth_shade_apply(h, ref, d24.data_ptr(), 16, d16.data_ptr(), out.data_ptr()) == E
        check_after("bad shades")
        # the renderers' usual cases
        assert lib.nmi_render_points_depth(h, None, None, 5, mp, 1, 2.0, g, out.data_ptr(), None, None) == E
        assert lib.nmi_render_points_depth(h, dp.data_ptr(), None, -1, mp, 1, 2.0, g, out.data_ptr(), None, None) == E
        assert lib.nmi_render_points_depth(h, dp.data_ptr(), None, 5, None, 1, 2.0, g, out.data_ptr(), None, None) == E
        assert lib.nmi_render_points_depth(h, dp.data_ptr(), None, 5, mp, 1, 2.0, g, None, None, None) == E
        assert lib.nmi_render_points_depth(h, dp.data_ptr(), None, 5, mp, 1, float("nan"), g, out.data_ptr(), None, None) == E
        assert lib.nmi_render_mesh_depth(h, None, T, mp, 1, g, out.data_ptr(), None, None) == E
        assert lib.nmi_render_mesh_depth(h, dx.data_ptr(), -1, mp, 1, g, out.data_ptr(), None, None) == E
        assert lib.nmi_render_mesh_depth(h, dx.data_ptr(), T, None, 1, g, out.data_ptr(), None, None) == E
        assert lib.nmi_render_mesh_depth(h, dx.data_ptr(), T, mp, 1, g, None, None, None) == E
        for S in (0, -1):
            assert lib.nmi_render_points_depth(h, dp.data_ptr(), None, 5, mp, S, 2.0, g, out.data_ptr(), None, None) == E
            assert lib.nmi_render_mesh_depth(h, dx.data_ptr(), T, mp, S, g, out.data_ptr(), None, None) == E
        assert lib.nmi_depth_shade_apply(h, g, None, 16, d16.data_ptr(), out.data_ptr()) == E
        assert lib.nmi_depth_shade_apply(h, g, d24.data_ptr(), -1, d16.data_ptr(), out.data_ptr()) == E
        check_after("bad renderer arguments")
        assert lib.nmi_depth_shade_apply(h, g, None, 0, None, None) == 0        # nothing to do is not an error
