"""Edges of the warp-stack producer: every device path against the fp32 twin (oracle/warp_oracle_np.py, == on bytes) and against
the float64 model (synthetic.warp_perspective_value) on hard homographies (tests/helpers/warp_cases.py): horizons in view,
180-degree rolls, mirrors, strong zooms, patches at the LDS budget, shifts onto the range bounds, warps out of reach, and
matrices scaled by powers of two and by extreme constants.  Plus the rejection of non-finite and singular matrices.

Paths: nmi_warp_kernel (global taps; dword and byte stores), nmi_warp_lds_kernel (warp_lds_block: staged, nothing-in-reach,
over-budget and bad-corner blocks), the warp blocks fused into level kernels (point-cloud front kernel, mesh bin and pairs
kernels), the side-branch warp of a level whose width is not a multiple of 16, and nmi_warp_mask_kernel.

The float64 criterion.  At every pixel whose float64 value lies more than tau(p) from a rounding tie (k + 1/2) the
product's byte equals the rounded float64 value; elsewhere it is within 1; fewer than 1 % of the pixels are that close
to a tie (counted away from the frame's border).  tau(p) is derived, not tuned.  The product computes the source coordinate in fp32:
test_tau_bounds_the_fp32_error checks |dx| + |dy| <= RHO = 2^-11 pixel against float64 for every family on the pixels in
reach (the largest error is ~4.7e-4, at 1248 columns, where the fp32 spacing is 2^-13).  The bilinear value is continuous
and moves by at most R(p) per pixel in x and in y, R(p) the range of the taps (zero border included) in the 4 x 4 window
around the pixel's source cell, which holds the cells an error below one pixel can reach.  So the coordinate error moves
the value by <= R(p) * RHO; the four fp32 products and sums add < 8 ulp of 255 < 2^-12.  Hence
tau(p) = R(p) * RHO + 2^-12.  A fixed tau of 1/16 would exclude 1/8 of all pixels with a fractional value; on the
criterion frame (smooth_frame: values multiples of 4, slope ~1 per pixel, so R = 4 or 8 away from the frame's border)
tau is ~0.004.  The multiples of 4 keep half- and quarter-pixel shifts (weights 1/2, 1/4) off exact ties.  The byte-exact
comparisons with the twin use a noisy frame (camera_frame), where a wrong tap shows.
"""
import numpy as np
import pytest

from helpers import masked_np as mnp
from helpers import warp_cases as wc
from oracle import warp_oracle_np as wo
from orbslam2_nmi_amd import capi, synthetic as sy

try:
    import torch
except ImportError:  # the CPU tier does not need it
    torch = None

f32 = np.float32
RHO = 2.0 ** -11

LDS_SIZES = [(16, 1), (16, 33), (48, 7), (144, 40), (640, 480), (848, 480), (1248, 376)]
GLOBAL_SIZES = [(1241, 376), (333, 97), (17, 5), (1, 1)]
REACH_SIZES = {(640, 480), (848, 480), (1248, 376)}   # frames large enough for every family to reach its branches


def smooth_frame(W, H):
    """Slowly varying pattern (slope < 1.1 per pixel), values multiples of 4."""
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    v = 128 + 60 * np.sin(x / 97 + 0.3) * np.cos(y / 83) + 50 * np.sin((x + y) / 151)
    return (4 * np.rint(v / 4)).astype(np.uint8)


def noisy_frame(W, H, seed=11):
    return sy.camera_frame(sy.scene(max(W, 64), max(H, 64), seed)[:H, :W], seed + 1)


def tap_range(img, u, v):
    """-> (R(p): max - min of the taps, zero border included, in the 4 x 4 window around the float64 source cell of every
    pixel, 0 where the source is out of reach (the value is 0 exactly on both sides); where that window lies inside the
    frame)"""
    h, w = img.shape
    pad = np.zeros((h + 8, w + 8), np.int32)
    pad[4:-4, 4:-4] = img
    win = [pad[dy:dy + h + 5, dx:dx + w + 5] for dy in range(4) for dx in range(4)]
    rng = np.max(win, 0) - np.min(win, 0)              # rng[j, i]: window with rows j - 4 .. j - 1, columns i - 4 .. i - 1
    with np.errstate(invalid="ignore"):
        reach = np.isfinite(u) & np.isfinite(v) & (u > -3) & (u < w + 2) & (v > -3) & (v < h + 2)
    x0 = np.floor(np.where(reach, u, 0)).astype(int)
    y0 = np.floor(np.where(reach, v, 0)).astype(int)
    inner = reach & (x0 >= 1) & (x0 <= w - 3) & (y0 >= 1) & (y0 <= h - 3)   # the window lies inside the frame
    return np.where(reach, rng[y0 + 3, x0 + 3], 0), inner   # rows y0 - 1 .. y0 + 2, columns x0 - 1 .. x0 + 2


def assert_float64_criterion(got, img, M, what=""):
    h, w = img.shape
    val = sy.warp_perspective_value(img, M)
    undefined = ~np.isfinite(val)                     # den == 0 exactly: both sides give 0
    val = np.where(undefined, 0.0, val)
    ref = np.clip(np.rint(val), 0, 255).astype(int)
    _, _, u, v = source_coords(M, w, h)
    r, inner = tap_range(img, u, v)
    tau = r * RHO + 2.0 ** -12
    near = (np.abs(val - np.floor(val) - 0.5) <= tau) | undefined
    d = got.astype(int) - ref
    assert np.abs(d).max(initial=0) <= 1, f"{what}: differs from the float64 model by {np.abs(d).max()}"
    assert (d[~near] == 0).all(), f"{what}: {(d[~near] != 0).sum()} pixels farther than tau from a tie differ"
    # counted where the window lies inside the frame: next to the zero border the jump to 0 makes tau large, and in frames
    # of a few rows or columns nearly every window meets it
    n_in = int(inner.sum())
    assert n_in < 1000 or (near & inner).sum() < 0.01 * n_in, f"{what}: {(near & inner).sum() / n_in:.2%} of the pixels excluded"


def source_coords(M, W, H):
    """-> (fp32 xs, ys as the twin and the kernels compute them, float64 u, v)"""
    c = wo.device_coeffs(M)
    yy, xx = np.mgrid[0:H, 0:W]
    fx, fy = xx.astype(f32), yy.astype(f32)
    Mi = np.linalg.inv(M)
    X, Y = xx.astype(np.float64), yy.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        co = f32(1.0) / ((c[6] * fx + c[7] * fy) + c[8])
        xs, ys = co * ((c[0] * fx + c[1] * fy) + c[2]), co * ((c[3] * fx + c[4] * fy) + c[5])
        d = Mi[2, 0] * X + Mi[2, 1] * Y + Mi[2, 2]
        u, v = (Mi[0, 0] * X + Mi[0, 1] * Y + Mi[0, 2]) / d, (Mi[1, 0] * X + Mi[1, 1] * Y + Mi[1, 2]) / d
    return xs, ys, u, v


# ----------------------------------------------------------------------------------------------------- CPU tier: the twin
CPU_SIZES = [(320, 240), (1248, 376), (17, 5)]


@pytest.mark.parametrize("family", list(wc.EXPECTED_BRANCHES))
@pytest.mark.parametrize("shape", CPU_SIZES, ids=[f"{w}x{h}" for w, h in CPU_SIZES])
def test_twin_meets_float64_criterion(family, shape):
    W, H = shape
    img = smooth_frame(W, H)
    for i, M in enumerate(wc.families(W, H)[family]):
        assert_float64_criterion(wo.warp_perspective(img, M), img, M, f"{family}[{i}]")


def test_tau_bounds_the_fp32_error():
    for W, H in CPU_SIZES + [(640, 480)]:
        for fam, lst in wc.families(W, H).items():
            for M in lst:
                xs, ys, u, v = source_coords(M, W, H)
                reach = np.isfinite(u) & np.isfinite(v) & (u > -3) & (u < W + 2) & (v > -3) & (v < H + 2)
                err = np.abs(xs - u)[reach].max(initial=0) + np.abs(ys - v)[reach].max(initial=0)
                assert err <= RHO, (W, H, fam, err)


def test_staging_branches_cover_every_branch():
    for W, H in sorted(REACH_SIZES):
        total = dict.fromkeys(wc.BRANCHES, 0)
        fams = wc.families(W, H)
        for fam, lst in fams.items():
            for M in lst:
                for b, n in wc.staging_branches(M, W, H).items():
                    total[b] += n
            assert wc.EXPECTED_BRANCHES[fam] <= wc.branches_reached(lst, W, H), (W, H, fam)
        assert all(total[b] > 0 for b in wc.BRANCHES), (W, H, total)
        # the budget pair straddles the limit: the first zoom's largest staged patch is within 1 KiB of it, the second goes over
        under, over = (wc.staging_branches(M, W, H, sizes=True) for M in fams["budget"])
        assert under["over"] == 0 and under["max_staged"] > wc.PATCH_BYTES - 1024 and over["over"] > 0


def test_device_coeffs_normalises_and_rejects():
    W, H = 640, 480
    for M in list(wc.families(W, H)["grid"]) + wc.scale_bases(W, H):
        c, ref = wo.device_coeffs(M), wo.inverse_coeffs_adjugate(M)
        assert 1 <= np.abs(c).max() < 2
        k = int(np.frexp(np.abs(c).max())[1] - np.frexp(np.abs(ref).max())[1])
        assert (c.view(np.uint32) == np.ldexp(ref, k).astype(f32).view(np.uint32)).all()   # the same bits up to 2^k
        for k in wc.SCALES_POW2:
            assert (wo.device_coeffs(np.ldexp(M, k)).view(np.uint32) == c.view(np.uint32)).all()
        for s in wc.SCALES_EXTREME:
            cs = wo.device_coeffs(s * M)
            assert np.isfinite(cs).all() and 1 <= np.abs(cs).max() < 2
            r = np.abs(c).max() / np.abs(cs).max()   # the same matrix up to scale
            assert np.allclose(cs * r, c, rtol=1e-6, atol=1e-6)
    for M in rejected_list(wc.scale_bases(W, H)[0]).values():
        with pytest.raises(ValueError):
            wo.device_coeffs(M[-1])
    with pytest.raises(ValueError):
        wo.device_coeffs(np.zeros((3, 3)))


def rejected_list(good):
    """Wn = 3 lists whose LAST matrix the product must reject: singular (det == 0 exactly), a NaN entry, an inf entry."""
    sing = np.array([[1.0, 2, 3], [2, 4, 6], [0, 0, 1]])
    nan, inf = good.copy(), good.copy()
    nan[2, 2], inf[0, 1] = np.nan, np.inf
    return {name: np.stack([good, good, m]) for name, m in (("singular", sing), ("nan", nan), ("inf", inf))}


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


def cases_with_bases(W, H):
    """-> (names, matrices [n, 3, 3], index of each family's first matrix); matrices 0 and 1 are wc.scale_bases."""
    names, Ms, first = ["base0", "base1"], list(wc.scale_bases(W, H)), {}
    for fam, lst in wc.families(W, H).items():
        first[fam] = len(Ms)
        names += [f"{fam}[{i}]" for i in range(len(lst))]
        Ms += lst
    return names, np.stack(Ms), first


def check_stack(got, frame, names, Ms, what):
    exp = wo.warp_stack(frame, Ms)
    bad = [names[i] for i in range(len(Ms)) if not (got[i] == exp[i]).all()]
    assert not bad, f"{what}: differs from the fp32 twin in {bad}"


def check_scale_invariance(got, first, what):
    """warp(2^k M) == warp(M) bit for bit (got[0], got[1]: the warps of scale_bases)."""
    n = len(wc.SCALES_POW2)
    for b in range(2):
        for j, k in enumerate(wc.SCALES_POW2):
            assert (got[first["pow2"] + b * n + j] == got[b]).all(), f"{what}: base {b} scaled by 2^{k} changes the warp"


def assert_reached(names, Ms, W, H):
    if (W, H) not in REACH_SIZES:
        return
    for fam, exp in wc.EXPECTED_BRANCHES.items():
        lst = [M for n, M in zip(names, Ms) if n.startswith(fam + "[")]
        assert exp <= wc.branches_reached(lst, W, H), (fam, W, H)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", LDS_SIZES + GLOBAL_SIZES, ids=[f"{w}x{h}" for w, h in LDS_SIZES + GLOBAL_SIZES])
def test_gpu_warp_stack_families(nmi, shape):
    W, H = shape
    names, Ms, first = cases_with_bases(W, H)
    assert_reached(names, Ms, W, H)
    F, S = noisy_frame(W, H), smooth_frame(W, H)
    with nmi.NmiContext(W, H) as ctx:
        got = ctx.warp_stack(dev(F), Ms).cpu().numpy()
        got_s = ctx.warp_stack(dev(S), Ms).cpu().numpy()
    check_stack(got, F, names, Ms, f"{W}x{H}")
    check_scale_invariance(got, first, f"{W}x{H}")
    check_scale_invariance(got_s, first, f"{W}x{H} smooth")
    for i, (n, M) in enumerate(zip(names, Ms)):
        assert_float64_criterion(got_s[i], S, M, f"{W}x{H} {n}")


@pytest.mark.gpu
@pytest.mark.parametrize("frame_off,out_off,W,H", [(1, 0, 640, 480), (0, 1, 640, 480), (0, 4, 640, 480), (1, 0, 333, 97), (0, 1, 333, 97)],
                         ids=["640-frame+1-dword", "640-out+1-bytes", "640-out+4-staged", "333-frame+1", "333-out+1"])
def test_gpu_warp_stack_misaligned(nmi, frame_off, out_off, W, H):
    """A frame at byte offset 1 sends a 640-wide frame to nmi_warp_kernel's dword store; an output at offset 1 to its byte
    store; offset 4 keeps the staged kernel (it needs 4-byte output alignment only)."""
    names, Ms, first = cases_with_bases(W, H)
    F = noisy_frame(W, H)
    n = len(Ms) * W * H
    fbuf = torch.zeros(W * H + 16, dtype=torch.uint8, device="cuda")
    fbuf[frame_off:frame_off + W * H] = dev(F.reshape(-1))
    frame = fbuf[frame_off:frame_off + W * H].view(H, W)
    obuf = torch.full((n + 16,), 77, dtype=torch.uint8, device="cuda")
    out = obuf[out_off:out_off + n].view(len(Ms), H, W)
    assert frame.data_ptr() % 16 == frame_off and out.data_ptr() % 16 == out_off
    with nmi.NmiContext(W, H) as ctx:
        ctx.warp_stack(frame, Ms, out=out)
    got = out.cpu().numpy()
    check_stack(got, F, names, Ms, f"{W}x{H} frame+{frame_off} out+{out_off}")
    check_scale_invariance(got, first, "misaligned")
    rest = obuf.cpu().numpy()
    assert (rest[:out_off] == 77).all() and (rest[out_off + n:] == 77).all()   # nothing written outside the output


@pytest.mark.gpu
def test_gpu_warp_stack_many_warps(nmi):
    """Wn = 729 at 64x48: the warp index in the launch grid and in the coefficient offsets."""
    W, H = 64, 48
    names, Ms, _ = cases_with_bases(W, H)
    grid = sy.warp_homographies(sy.intrinsics(W, H), (9, 9, 9), (0.05, 0.05, 0.1))
    Ms = np.concatenate([Ms, grid])[:729]
    names = (names + [f"grid9[{i}]" for i in range(len(grid))])[:729]
    F = noisy_frame(W, H)
    with nmi.NmiContext(W, H) as ctx:
        got = ctx.warp_stack(dev(F), Ms).cpu().numpy()
    assert got.shape == (729, H, W)
    check_stack(got, F, names, Ms, "Wn=729")


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(640, 480), (333, 97), (48, 7)], ids=["640x480", "333x97", "48x7"])
@pytest.mark.parametrize("with_mask", [False, True], ids=["border", "frame-mask"])
def test_gpu_warp_stack_masked_families(nmi, shape, with_mask):
    W, H = shape
    names, Ms, first = cases_with_bases(W, H)
    F = noisy_frame(W, H)
    fm = None
    if with_mask:
        fm = np.ones((H, W), np.uint8)
        fm[H - max(1, H // 6):] = 0
        fm[:max(1, H // 8), :max(1, W // 10)] = 0
        fm[(np.arange(H)[:, None] * 7 + np.arange(W)[None, :] * 3) % 53 == 0] = 0   # scattered holes
    F2 = F.copy()
    if fm is not None:   # the masked-out frame pixels randomised
        F2[fm == 0] = np.random.default_rng(5).integers(0, 256, int((fm == 0).sum()), dtype=np.uint8)
    with nmi.NmiContext(W, H) as ctx:
        ws, wm = ctx.warp_stack_masked(dev(F), Ms, None if fm is None else dev(fm))
        ws2, wm2 = ctx.warp_stack_masked(dev(F2), Ms, None if fm is None else dev(fm))
        plain = ctx.warp_stack(dev(F), Ms)
    ws, wm, ws2, wm2 = ws.cpu().numpy(), wm.cpu().numpy(), ws2.cpu().numpy(), wm2.cpu().numpy()
    assert (ws == plain.cpu().numpy()).all()
    check_stack(ws, F, names, Ms, f"masked {W}x{H}")
    exp = mnp.warp_masks((H, W), Ms, fm)
    bad = [names[i] for i in range(len(Ms)) if not (wm[i] == exp[i]).all()]
    assert not bad, f"masks differ from the twin in {bad}"
    assert (wm2 == wm).all()
    valid = wm != 0
    assert (ws2[valid] == ws[valid]).all(), "a valid pixel depends on a masked-out frame pixel"
    for i, M in enumerate(Ms):
        xs, ys, _, _ = source_coords(M, W, H)
        with np.errstate(invalid="ignore"):
            inside = (xs > -2) & (xs < W + 1) & (ys > -2) & (ys < H + 1)
        assert (ws[i][~inside] == 0).all() and (wm[i][~inside] == 0).all(), names[i]
    check_scale_invariance(wm, first, "masks")


# ---------------------------------------------------------------------------------------------- levels
def level_scene(nmi, ctx, W, H, mesh):
    """(xyz, attr, texture or None, device frame, mvps [4, 16]): a plane seen by a displaced camera."""
    from test_render import plane_cloud, plane_mesh
    if mesh:
        xyz, attr, rgb, rp = plane_mesh(W, H, nx=mesh[0], ny=mesh[1])
        tex = nmi.NmiTexture(ctx, rgb)
    else:
        xyz, attr, rp = plane_cloud(W, H, density=2.0)
        tex = None
    dx, da = dev(xyz), dev(attr)
    cam = ((0, 0, 0), (0, 0, 1), (0, -1, 0))
    view = capi.render_mvp(rp, *cam, (0.05, 0, 0))[None]
    fr = ctx.render_mesh(dx, da, tex, view)[0] if mesh else ctx.render_points(dx, torch.sqrt(da), view, 3.0)[0]
    frame = torch.flip(fr, dims=[0]).contiguous()
    mvps = np.stack([capi.render_mvp(rp, *cam, (0.02 * s, -0.01 * s, 0.0)) for s in range(4)])
    return dx, da, tex, frame, mvps


LEVELS = [  # id, W, H, mesh quads (nx, ny) or None, views
    ("cloud-fused-320x240", 320, 240, None, 4),          # width % 16 == 0: warp blocks in the front kernel
    ("cloud-side-324x240", 324, 240, None, 4),           # width % 16 != 0: nmi_warp_kernel on a side branch
    ("mesh-bin-320x240", 320, 240, (12, 9), 4),          # 225 triangles: nmi_mesh_bin_kernel
    ("mesh-pairs-640x480", 640, 480, (192, 160), 8),     # 61,449 triangles = 241 blocks x 8 views > 4 per CU: the pairs kernel
]


@pytest.mark.gpu
@pytest.mark.parametrize("lid,W,H,mesh,S", LEVELS, ids=[l[0] for l in LEVELS])
def test_gpu_level_warps_families(nmi, lid, W, H, mesh, S):
    names, Ms, first = cases_with_bases(W, H)
    with nmi.NmiContext(W, H) as ctx:
        dx, da, tex, frame, mvps = level_scene(nmi, ctx, W, H, mesh)
        mvps = np.concatenate([mvps] * (S // len(mvps)))
        with nmi.NmiLevel(ctx, dx, da, frame, S, len(Ms), 3.0, texture=tex) as lv:
            lv.run(mvps, Ms)
            _, ws, t = lv.outputs()
        F = frame.cpu().numpy()
    assert_reached(names, Ms, W, H)
    check_stack(ws, F, names, Ms, lid)
    check_scale_invariance(ws, first, lid)
    assert np.isfinite(t).all()


@pytest.mark.gpu
@pytest.mark.parametrize("mesh", [None, (12, 9)], ids=["cloud", "mesh"])
def test_gpu_level_extreme_scales(nmi, mesh):
    """s M for the extreme s: the level's fused warps equal the twin's, and nmi_warp_stack meets the float64 criterion."""
    W, H = 320, 240
    bases = wc.scale_bases(W, H)
    Ms = np.stack([s * M for M in bases for s in wc.SCALES_EXTREME])
    with nmi.NmiContext(W, H) as ctx:
        dx, da, tex, frame, mvps = level_scene(nmi, ctx, W, H, mesh)
        with nmi.NmiLevel(ctx, dx, da, frame, len(mvps), len(Ms), 3.0, texture=tex) as lv:
            lv.run(mvps, Ms)
            _, ws, _ = lv.outputs()
        F = frame.cpu().numpy()
    check_stack(ws, F, [f"base{i // len(wc.SCALES_EXTREME)} * {s}" for i, s in enumerate(wc.SCALES_EXTREME * 2)], Ms, "level")
    S = smooth_frame(W, H)
    with nmi.NmiContext(W, H) as ctx:
        got = ctx.warp_stack(dev(S), Ms).cpu().numpy()
    for i, M in enumerate(Ms):
        assert_float64_criterion(got[i], S, M, f"extreme {i}")


# ---------------------------------------------------------------------------------------------- rejection
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["singular", "nan", "inf"])
def test_gpu_warp_stack_rejects(nmi, kind):
    W, H = 64, 48
    Ms = rejected_list(wc.scale_bases(W, H)[0])[kind]
    F = noisy_frame(W, H)
    with nmi.NmiContext(W, H) as ctx:
        for call in (ctx.warp_stack, ctx.warp_stack_masked):
            with pytest.raises(capi.NmiError) as e:
                call(dev(F), Ms)
            assert e.value.code == capi.ERR_INVALID_ARGUMENT
        # the context stays usable: an accepted list right after gives the twin's bytes
        assert (ctx.warp_stack(dev(F), Ms[:2]).cpu().numpy() == wo.warp_stack(F, Ms[:2])).all()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["singular", "nan", "inf"])
def test_gpu_level_rejects_and_keeps_state(nmi, kind):
    """A rejected nmi_level_run changes nothing: the next run's renders, warps, ratings and winner are those of the same run
    without the rejected call."""
    W, H = 320, 240
    with nmi.NmiContext(W, H) as ctx:
        dx, da, tex, frame, mvps = level_scene(nmi, ctx, W, H, None)
        A = np.stack(wc.scale_bases(W, H) + [wc.shift(1.5, -2)])
        B = np.stack([wc.rotation(W, H, yaw=3), wc.shift(-4, 0.5), wc.rotation(W, H, roll=-2)])
        bad = rejected_list(A[0])[kind]
        with nmi.NmiLevel(ctx, dx, da, frame, len(mvps), 3, 3.0) as lv:
            lv.run(mvps, A)
            win_ref = lv.run(mvps, B)
            out_ref = lv.outputs()
            lv.run(mvps, A)
            with pytest.raises(capi.NmiError) as e:
                lv.run(mvps, bad)
            assert e.value.code == capi.ERR_INVALID_ARGUMENT
            win = lv.run(mvps, B)
            out = lv.outputs()
    assert win[0] == win_ref[0] and np.float32(win[1]).view(np.uint32) == np.float32(win_ref[1]).view(np.uint32)
    for a, b in zip(out, out_ref):
        assert (a.view(np.uint8) == b.view(np.uint8)).all()
