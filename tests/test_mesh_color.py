"""Vertex-coloured meshes (nmi_render_mesh_colored, coloured mesh levels, nmi_map_load_obj_colored).

The twin (tests/helpers/mesh_color.py) is oracle/mesh_oracle_np.render_staged with the colour in u's place and the point renderer's
colour rule on the interpolated value; np.float64 gives the model.  CPU tier: known answers on the twin, the twin against the float64
model, the loader.  GPU tier: every coloured entry of the library against the twin, `==` on every byte -- the coloured shader takes
no logarithm, so test_mesh_edges' one-grey-level allowance for minified pixels has nothing to apply to.

Twin against model (test_twin_meets_float64_model): on the pixels mesh_bounds.compare_view does not exempt for coverage or winner,
|grey32 - grey64| <= 255 E_u + 1 with E_u the bound mesh_bounds.shade_ev carries for u -- test_mesh_edges' grey criterion with the
texture's Lipschitz constant replaced by 1 (grey = round(255 clamp(c)); the clamp does not stretch, the two roundings add at most
1).  Of every family's bulk fragments at most BULK_EXEMPT may be exempt, the cap and the scope test_mesh_edges holds on these same
meshes (far_from_origin at 1,000 m is printed, not asserted, there and here).
"""
import ctypes as C
import functools
import os
import subprocess
import time

import numpy as np
import pytest

from conftest import ROOT
from helpers import mesh_cases as mc
from helpers import mesh_color as col
from helpers import render_cases as rc

try:
    import torch
except ImportError:  # the CPU tier does not need it
    torch = None

f32 = np.float32
BULK_EXEMPT = 0.02                  # test_mesh_edges.BULK_EXEMPT
HEAVY = {"full_bins", "frustum_margin", "far_from_origin", "tessellation", "depth"}     # test_mesh_edges.HEAVY
GPU_SIZES = [(160, 120), (150, 90), (40, 30), (130, 129)]                                # test_mesh_edges.GPU_SIZES
FAMILIES = [f for f in mc.EXPECTED_BRANCHES if f != "huge_uv"]      # (huge_uv is about the texture wrap: no texture here)
CPU_SIZES = [(150, 90), (40, 30)]
KS = (0, 1, 37, 128, 254, 255)
SHIFT = (0.07, -0.05, 0.3)          # test_mesh_edges._replays' second replay


def test_constants_are_the_textured_tests():
    import test_mesh_edges as te
    assert (BULK_EXEMPT, HEAVY, GPU_SIZES) == (te.BULK_EXEMPT, te.HEAVY, te.GPU_SIZES)
    assert set(FAMILIES) | {"huge_uv"} == set(te.FAMILIES)


# ----------------------------------------------------------------------------------------------------- CPU tier
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("shape", CPU_SIZES, ids=[f"{w}x{h}" for w, h in CPU_SIZES])
def test_twin_constant_colour_known_answers(family, shape):
    """A constant colour k / 255 gives grey k on every covered pixel and 255 elsewhere (the interpolation of a constant is the
    constant to within far less than half a grey level, also through the near-plane clipper and reciprocal_range's division
    path); NaN gives 0; 2.0 and -1.0 give 255 and 0."""
    W, H = shape
    n_px = 0
    for i, c in enumerate(mc.family(family, W, H)):
        n = len(c["xyz"])
        for value, want in [(f32(k) / f32(255.0), k) for k in KS] + [(f32(np.nan), 0), (f32(2.0), 255), (f32(-1.0), 0)]:
            for s, m in enumerate(c["mvps"]):
                r = col.render(c["xyz"], np.full(n, value, f32), m, W, H)
                cov = r["covered"]
                assert (r["grey"][~cov] == 255).all()
                wrong = cov & (r["grey"] != want)
                assert not wrong.any(), f"{family}[{i}] view {s}, colour {value}: {int(wrong.sum())} of {int(cov.sum())} covered pixels are not {want}"
                n_px += int(cov.sum())
    print(f"{family} {W}x{H}: {n_px} covered pixels checked")
    assert n_px > 0


def _views(c):
    S = len(c["mvps"])
    if "distance" in c:
        return (3,)                       # (test_mesh_edges.analysed: far_from_origin takes the tessellation's last view)
    return range(S) if S <= 4 else sorted({0, S // 2, S - 1})


@functools.lru_cache(maxsize=None)
def _analysed(family, W, H):
    out = []
    for i, c in enumerate(mc.family(family, W, H)):
        if not c.get("criterion", True):        # (full_bins' fillers: test_mesh_edges.analysed leaves them to the kernels, too)
            continue
        for s in _views(c):
            r = col.compare_view(c["xyz"], col.colors_of(family, W, H, i), c["mvps"][s], W, H, c["bulk"])
            r.update(case=i, view=s, distance=c.get("distance"))
            out.append(r)
    return out


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("shape", CPU_SIZES, ids=[f"{w}x{h}" for w, h in CPU_SIZES])
def test_twin_meets_float64_model(family, shape):
    W, H = shape
    if family in HEAVY and shape != (150, 90):
        return      # (HEAVY: one size, as in test_mesh_edges)
    res = _analysed(family, W, H)
    bad = [f"[{r['case']}] view {r['view']}: {p}" for r in res for p in r["problems"] + r["grey_problems"]]
    print(f"{family} {W}x{H}: grey compared on {sum(r['pixels'] for r in res)} pixels, largest difference {max([r['worst'] for r in res] + [0])}, "
          f"{sum(r['unbounded'] for r in res)} more without a finite bound")
    assert not bad, bad[:8]
    for dist in sorted({r["distance"] for r in res}, key=lambda d: -1 if d is None else d):
        sel = [r for r in res if r["distance"] == dist]
        n, n_ex = sum(r["frags"] for r in sel), sum(r["frags_exempt"] for r in sel)
        print(f"{family} {W}x{H}" + (f" at {dist:g} m" if dist is not None else "") + f": {n_ex} of {n} bulk fragments exempt")
        if dist is not None and dist >= 1000.0:
            continue
        assert n_ex <= BULK_EXEMPT * n, f"{family}: {n_ex} of {n} fragments off the boundaries exempt"


def test_seeded_colours_reach_both_clamps_and_the_nonfinite_ones():
    W, H = 150, 90
    for family in FAMILIES:
        allc = np.concatenate([col.colors_of(family, W, H, i) for i in range(len(mc.family(family, W, H)))])
        fin = allc[np.isfinite(allc)]
        assert fin.min() < 0 and fin.max() > 1 and fin.min() >= -0.1 and fin.max() <= 1.1, family
        assert np.isfinite(allc).all() == (family != "nonfinite")
    c = col.colors_of("nonfinite", W, H, 0)
    assert np.isnan(c).any() and (c == np.inf).any() and (c == -np.inf).any()


# ---- loader
QUAD_OBJ = """# a quad with four colours, every face index form
v 0 0 0 1 0 0
v 1 0 0 0 1 0
vt 0.5 0.5
v 1 1 0 0.25 0.5 0.75
vn 0 0 1
v 0 1 0.5 0.125 1 0
f 1 2 3
f 1/1 3/1 4/1
f 4//1 3//1 2//1
f 2/1/1 1/1/1 4/1/1
"""
QUAD_V = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0.5]], f32)
QUAD_C = np.array([[1, 0, 0], [0, 1, 0], [0.25, 0.5, 0.75], [0.125, 1, 0]], f32)
QUAD_F = np.array([[1, 2, 3], [1, 3, 4], [4, 3, 2], [2, 1, 4]]) - 1


@pytest.fixture(scope="module")
def host():
    from orbslam2_nmi_amd import build as nmi_build
    from orbslam2_nmi_amd import hostapi
    nmi_build.build()
    return hostapi


def _load_rc(host, path):
    xyz, red, rgb, n = C.POINTER(C.c_float)(), C.POINTER(C.c_float)(), C.POINTER(C.c_float)(), C.c_int64()
    rc_ = host._lib().nmi_map_load_obj_colored(str(path).encode(), C.byref(xyz), C.byref(red), C.byref(rgb), C.byref(n))
    assert rc_ != 0 and not xyz and not red and not rgb and n.value == 0
    return rc_


def test_loader_colored_obj(host, tmp_path):
    p = tmp_path / "quad.obj"
    p.write_text(QUAD_OBJ)
    xyz, red, rgb = host.load_obj_colored(p)
    idx = QUAD_F.reshape(-1)
    assert xyz.dtype == f32 and xyz.shape == (12, 3) and (xyz == QUAD_V[idx]).all()
    assert red.shape == (12,) and (red == QUAD_C[idx, 0]).all()
    assert rgb.shape == (12, 3) and (rgb == QUAD_C[idx]).all()
    # rgb is optional
    x2, r2, n = C.POINTER(C.c_float)(), C.POINTER(C.c_float)(), C.c_int64()
    assert host._lib().nmi_map_load_obj_colored(str(p).encode(), C.byref(x2), C.byref(r2), None, C.byref(n)) == 0 and n.value == 12
    assert (np.ctypeslib.as_array(r2, shape=(12,)) == red).all()
    host._lib().nmi_map_free(C.cast(x2, C.c_void_p)), host._lib().nmi_map_free(C.cast(r2, C.c_void_p))
    # the three failures, by the loaders' codes: -2 not in the format, -3 index outside the lists, -5 not readable
    (tmp_path / "plain.obj").write_text(QUAD_OBJ.replace("v 1 0 0 0 1 0", "v 1 0 0"))
    assert _load_rc(host, tmp_path / "plain.obj") == -2
    (tmp_path / "range.obj").write_text(QUAD_OBJ + "f 1 2 5\n")
    assert _load_rc(host, tmp_path / "range.obj") == -3
    (tmp_path / "zero.obj").write_text(QUAD_OBJ + "f 0 1 2\n")
    assert _load_rc(host, tmp_path / "zero.obj") == -3
    assert _load_rc(host, tmp_path / "missing.obj") == -5
    (tmp_path / "quadface.obj").write_text(QUAD_OBJ + "f 1 2 3 4\n")
    assert _load_rc(host, tmp_path / "quadface.obj") == -2
    with pytest.raises(ValueError):
        host.load_obj_colored(tmp_path / "missing.obj")


def test_loader_under_asan_ubsan(tmp_path):
    """The loader as a stand-alone program under AddressSanitizer + UBSan on well-formed and hostile files (the pattern of
    test_host_sanitizers.py: nothing is preloaded into python)."""
    exe = tmp_path / "map_color_sanitize"
    host = os.path.join(ROOT, "orbslam2_nmi_amd", "host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), "-I" + host, os.path.join(ROOT, "tests", "native", "map_color_sanitize.cpp"),
                           os.path.join(host, "nmi_map_color.cpp"), os.path.join(host, "nmi_map.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", TMPDIR=str(tmp_path)))
    assert r.returncode == 0, r.stdout + r.stderr
    assert "map color sanitize ok" in r.stdout


# ----------------------------------------------------------------------------------------------------- GPU tier
@pytest.fixture(scope="module")
def nmi():
    if torch is None or not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    import orbslam2_nmi_amd as m
    m.load_library()
    return m


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def differs(tag, got, twins, masks=None):
    """`==` on every byte of a render stack (and of its coverage masks) against the twin's -> list of complaints."""
    bad = []
    for s, t in enumerate(twins):
        d = got[s] != t["grey"]
        if d.any():
            yy, xx = np.nonzero(d)
            bad.append(f"{tag} view {s}: {int(d.sum())} px differ, first ({xx[0]}, {yy[0]}): got {got[s][yy[0], xx[0]]} twin {t['grey'][yy[0], xx[0]]}")
        if masks is not None and not (masks[s] == t["covered"].astype(np.uint8)).all():
            bad.append(f"{tag} view {s}: {int((masks[s] != t['covered']).sum())} mask px differ")
    return bad


GPU_CASES = [(f, s) for f in FAMILIES for s in GPU_SIZES if f not in HEAVY or s == (150, 90)]
GPU_IDS = [f"{s[0]}x{s[1]}-{f}" for f, s in GPU_CASES]


@pytest.mark.gpu
@pytest.mark.parametrize("family,shape", GPU_CASES, ids=GPU_IDS)
def test_gpu_render_mesh_colored_families(nmi, family, shape):
    """nmi_render_mesh_colored and _masked against the twin (the masked render byte-equal to the plain one, the masks the twin's
    coverage), one image whatever the tile queue's and the clip queue's capacity, and the mesh after nmi_sort_triangles_colored
    against the twin of the SORTED arrays."""
    W, H = shape
    bad = []
    t0 = time.time()
    with nmi.NmiContext(W, H) as ctx:
        for i, c in enumerate(mc.family(family, W, H)):
            tag = f"{family}[{i}]"
            colors = col.colors_of(family, W, H, i)
            twins = col.twin_of(family, W, H, i)
            dx, dc = dev(c["xyz"]), dev(colors)
            got = ctx.render_mesh_colored(dx, dc, c["mvps"]).cpu().numpy()
            bad += differs(tag + " render", got, twins)
            r2, m2 = ctx.render_mesh_colored_masked(dx, dc, c["mvps"])
            if not (r2.cpu().numpy() == got).all():
                bad.append(f"{tag}: the masked render differs from the plain one")
            bad += differs(tag + " masked", r2.cpu().numpy(), twins, m2.cpu().numpy())
            for cap, clip_cap in ((5, 1 << 18), (0, 1 << 18), (4 << 20, 2)):
                ctx.set_option(ctx.OPT_TILE_QUEUE, cap)
                ctx.set_option(ctx.OPT_CLIP_QUEUE, clip_cap)
                if not (ctx.render_mesh_colored(dx, dc, c["mvps"]).cpu().numpy() == got).all():
                    bad.append(f"{tag}: tile queue {cap} / clip queue {clip_cap} gives another image")
            ctx.set_option(ctx.OPT_TILE_QUEUE, 4 << 20)
            ctx.set_option(ctx.OPT_CLIP_QUEUE, 1 << 18)
            sx, sc = ctx.sort_triangles_colored(dx, dc)
            hx, hc = sx.cpu().numpy(), sc.cpu().numpy()
            T = len(hx) // 3
            rec = lambda x, k: np.concatenate([x.reshape(T, 9), k.reshape(T, 3)], 1).view(np.uint32)     # noqa: E731
            if sorted(map(bytes, rec(hx, hc))) != sorted(map(bytes, rec(c["xyz"], colors))):
                bad.append(f"{tag}: the sorted mesh is not a permutation of the triangles with their colours")
            bad += differs(tag + " sorted", ctx.render_mesh_colored(sx, sc, c["mvps"]).cpu().numpy(), col.render_stack(hx, hc, c["mvps"], W, H))
    print(f"{family} {W}x{H}: {time.time() - t0:.1f} s")
    assert not bad, bad[:10]


@pytest.mark.gpu
@pytest.mark.parametrize("family,shape", GPU_CASES, ids=GPU_IDS)
def test_gpu_colored_level_families(nmi, family, shape):
    """A coloured mesh NmiLevel, plain and covered, over three replays with changing matrices: renders and coverage equal the twin
    each replay.  A textured level created, run and destroyed on the same context in between gives the render it gave before the
    first coloured level: the coloured kernels leave the work area clean."""
    W, H = shape
    bad = []
    with nmi.NmiContext(W, H) as ctx:
        frame = dev(np.random.default_rng(0).integers(0, 256, (H, W), dtype=np.uint8))
        for i, c in enumerate(mc.family(family, W, H)):
            dx, dc, du = dev(c["xyz"]), dev(col.colors_of(family, W, H, i)), dev(c["uv"])
            S = len(c["mvps"])
            replays = [c["mvps"], rc.shifted(c["mvps"], SHIFT), c["mvps"]]
            assert all(not np.array_equal(a, b) for a, b in zip(replays[0], replays[1])), "a replay's view did not change"
            twins = [col.twin_of(family, W, H, i), col.twin_of(family, W, H, i, SHIFT), col.twin_of(family, W, H, i)]

            def textured(tex):
                with nmi.NmiLevel(ctx, dx, du, frame, S, 1, 1.0, texture=tex) as lv:
                    lv.run(c["mvps"], np.eye(3)[None])
                    return lv.outputs()[0]

            with nmi.NmiTexture(ctx, c["rgb"]) as tex:
                before = textured(tex)
                for covered in (False, True):
                    with nmi.NmiLevel(ctx, dx, dc, frame, S, 1, 1.0, colors=True) as lv:
                        if covered:
                            lv.set_coverage(True)
                        for rep, mv in enumerate(replays):
                            lv.run(mv, np.eye(3)[None])
                            tag = f"{family}[{i}] {'covered ' if covered else ''}level replay {rep}"
                            bad += differs(tag, lv.outputs()[0], twins[rep], lv.coverage()[0] if covered else None)
                    if not (textured(tex) == before).all():
                        bad.append(f"{family}[{i}]: a textured level after the {'covered' if covered else 'plain'} coloured one renders another image")
    assert not bad, bad[:10]


@pytest.mark.gpu
def test_gpu_colored_pairs_pass_vs_twin(nmi):
    """The two-kernel binning pass (nmi_mesh_cull_kernel + nmi_mesh_bin_pairs_kernel, which serve both kinds of mesh) in front of the
    coloured tile kernel: the 4,800-triangle tessellation under 64 views at 160 x 120, as test_mesh_edges.test_gpu_mesh_pairs_pass_vs_twin builds it, with colours.
    launch_render_mesh takes that pass when nblocks * views > 4 * compute units (asserted for the device at hand).
    Every byte of all 64 views and their masks is checked: every eighth view against the twin (the twin of all 64 is half a minute
    of Python, which that test already spends on the same geometry), and all 64 against the same view rendered alone, S = 1 --
    19 pairs, the one-kernel binning pass, which test_gpu_render_mesh_colored_families holds to the twin.  What the pairs pass can
    get wrong is which (block of triangles, view) pairs reach the bins; a pair lost or doubled shows in that view either way."""
    W, H = 160, 120
    views = np.concatenate([rc.shifted(mc.tessellation_views(W, H)[:1], (0.4 * np.sin(0.7 * s), 0.3 * np.cos(1.1 * s), 0.05 * s - 1.0)) for s in range(64)])
    xyz, _, _ = mc.tessellation_mesh(W, H, views[0], nx=40, ny=30, seed=8)
    xyz = np.ascontiguousarray(xyz.astype(f32))
    assert len(xyz) // 3 == 4800
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert ((4800 + 255) // 256) * 64 > 4 * cus, cus
    assert (4800 + 255) // 256 <= 4 * cus, cus          # ... and one view alone does not take it
    colors = np.random.default_rng(8).uniform(-0.1, 1.1, len(xyz)).astype(f32)
    some = list(range(0, 64, 8))
    t0 = time.time()
    twins = col.render_stack(xyz, colors, views[some], W, H)
    print(f"twin of {len(some)} views: {time.time() - t0:.0f} s")
    assert sum(int(t["covered"].sum()) for t in twins) > 0.2 * len(some) * W * H
    with nmi.NmiContext(W, H) as ctx:
        dx, dc = dev(xyz), dev(colors)
        got, mask = ctx.render_mesh_colored_masked(dx, dc, views)
        got, mask = got.cpu().numpy(), mask.cpu().numpy()
        bad = differs("pairs pass", got[some], twins, mask[some])
        for s in range(64):
            g1, m1 = ctx.render_mesh_colored_masked(dx, dc, views[s:s + 1])
            if not ((g1.cpu().numpy()[0] == got[s]).all() and (m1.cpu().numpy()[0] == mask[s]).all()):
                bad.append(f"view {s}: the pairs pass and the one-kernel pass render different images")
    assert not bad, bad[:10]


@pytest.mark.gpu
def test_gpu_colored_level_equals_separate_calls(nmi):
    """On the 8 x 6 tessellation at 160 x 120, S = 9, Wn = 4: the rating table and winner of a coloured level are bit-equal to
    nmi_search_grid over nmi_render_mesh_colored + nmi_warp_stack; a _block level over renders [3, 7) x warps [1, 3) returns the whole
    table's cells with global indices, and that block's winner."""
    from orbslam2_nmi_amd import capi
    from orbslam2_nmi_amd import synthetic as sy
    W, H = 160, 120
    S, Wn = 9, 4
    c = mc.family("tessellation", W, H)[0]
    assert len(c["xyz"]) // 3 == 2 * 2 * 8 * 6
    colors = col.colors_of("tessellation", W, H, 0)
    mvps = np.concatenate([rc.shifted(c["mvps"][:1], (0.03 * (s % 3 - 1), 0.02 * (s // 3 - 1), 0.0)) for s in range(S)])
    Ms = capi.warp_homographies(sy.intrinsics(W, H), (2, 2, 1), (0.02, 0.02, 0.05))
    assert len(Ms) == Wn
    with nmi.NmiContext(W, H) as ctx:
        dx, dc = dev(c["xyz"]), dev(colors)
        fr = ctx.render_mesh_colored(dx, dc, rc.shifted(c["mvps"][:1], (0.01, 0.0, 0.0)))[0]
        frame = torch.flip(fr, dims=[0]).contiguous()
        rs = ctx.render_mesh_colored(dx, dc, mvps)
        ws = ctx.warp_stack(frame, Ms)
        table = torch.zeros(Wn, S, dtype=torch.float32, device="cuda")
        want = ctx.search_grid(rs, ws, table)
        table = table.cpu().numpy()
        assert len(np.unique(table)) > S * Wn // 2, "the ratings do not tell the cells apart"
        with nmi.NmiLevel(ctx, dx, dc, frame, S, Wn, 1.0, colors=True) as lv:
            for _ in range(2):
                got = lv.run(mvps, Ms)
                r, v, t = lv.outputs()
                assert (r == rs.cpu().numpy()).all() and (v == ws.cpu().numpy()).all()
                assert (t.view(np.uint32) == table.view(np.uint32)).all()
                assert got[0] == want[0] and np.float32(got[1]).view(np.uint32) == np.float32(want[1]).view(np.uint32), (got, want)
        s0, s1, w0, w1 = 3, 7, 1, 3
        with nmi.NmiLevel(ctx, dx, dc, frame, s1 - s0, w1 - w0, 1.0, colors=True, block=(s0, S, w0, Wn)) as blk:
            got = blk.run(mvps[s0:s1], Ms[w0:w1])
            t = blk.outputs()[2]
            cells = table[w0:w1, s0:s1]
            assert (t.view(np.uint32) == cells.view(np.uint32)).all()
            best = cells.max()
            ww, ss = np.nonzero(cells == best)
            index = int(min((w0 + a) * S + (s0 + b) for a, b in zip(ww, ss)))      # equal scores: the lower global index wins
            assert got[0] == index and np.float32(got[1]).view(np.uint32) == best.view(np.uint32), (got, index, best)


@pytest.mark.gpu
def test_gpu_colored_argument_errors(nmi):
    """NMI_ERR_INVALID_ARGUMENT, and nothing launched (the outputs keep their bytes): a null d_red with triangles to draw, S <= 0,
    aliasing outputs in the sort."""
    from orbslam2_nmi_amd import capi
    W, H = 40, 30
    c = mc.family("tessellation", W, H)[0]
    T = len(c["xyz"]) // 3
    with nmi.NmiContext(W, H) as ctx:
        lib, h = ctx._lib, ctx._h
        dx, dc = dev(c["xyz"]), dev(col.colors_of("tessellation", W, H, 0))
        out = torch.full((1, H, W), 7, dtype=torch.uint8, device="cuda")
        msk = torch.full((1, H, W), 7, dtype=torch.uint8, device="cuda")
        frame = torch.zeros((H, W), dtype=torch.uint8, device="cuda")
        m = np.ascontiguousarray(c["mvps"][:1], f32)
        mp = m.ctypes.data_as(C.POINTER(C.c_float))
        torch.cuda.synchronize()
        E = capi.ERR_INVALID_ARGUMENT
        assert lib.nmi_render_mesh_colored(h, dx.data_ptr(), None, T, mp, 1, out.data_ptr()) == E
        assert lib.nmi_render_mesh_colored_masked(h, dx.data_ptr(), None, T, mp, 1, out.data_ptr(), msk.data_ptr()) == E
        assert lib.nmi_render_mesh_colored_masked(h, dx.data_ptr(), dc.data_ptr(), T, mp, 1, out.data_ptr(), None) == E
        for S in (0, -1):
            assert lib.nmi_render_mesh_colored(h, dx.data_ptr(), dc.data_ptr(), T, mp, S, out.data_ptr()) == E
            assert lib.nmi_render_mesh_colored_masked(h, dx.data_ptr(), dc.data_ptr(), T, mp, S, out.data_ptr(), msk.data_ptr()) == E
            lv = C.c_void_p()
            assert lib.nmi_level_create_mesh_colored(h, dx.data_ptr(), dc.data_ptr(), T, frame.data_ptr(), S, 1, C.byref(lv)) == E and not lv.value
        lv = C.c_void_p()
        assert lib.nmi_level_create_mesh_colored(h, dx.data_ptr(), None, T, frame.data_ptr(), 1, 1, C.byref(lv)) == E and not lv.value
        assert lib.nmi_level_create_mesh_colored_block(h, dx.data_ptr(), None, T, frame.data_ptr(), 1, 0, 1, 1, 0, 1, C.byref(lv)) == E and not lv.value
        assert lib.nmi_level_create_mesh_colored_block(h, dx.data_ptr(), dc.data_ptr(), T, frame.data_ptr(), 2, 0, 1, 1, 0, 1, C.byref(lv)) == E and not lv.value
        ox, oc = torch.full_like(dx, 7.0), torch.full_like(dc, 7.0)
        keep_x, keep_c = dx.clone(), dc.clone()
        torch.cuda.synchronize()
        assert lib.nmi_sort_triangles_colored(h, dx.data_ptr(), dc.data_ptr(), T, dx.data_ptr(), oc.data_ptr()) == E
        assert lib.nmi_sort_triangles_colored(h, dx.data_ptr(), dc.data_ptr(), T, ox.data_ptr(), dc.data_ptr()) == E
        assert lib.nmi_sort_triangles_colored(h, dx.data_ptr(), None, T, ox.data_ptr(), oc.data_ptr()) == E
        ctx.synchronize()
        torch.cuda.synchronize()
        assert (out == 7).all() and (msk == 7).all() and (ox == 7).all() and (oc == 7).all()
        assert torch.equal(dx, keep_x) and torch.equal(dc, keep_c)
        # and the same context still renders
        got = ctx.render_mesh_colored(dx, dc, m).cpu().numpy()
        assert not differs("after the refused calls", got, col.twin_of("tessellation", W, H, 0)[:1])
