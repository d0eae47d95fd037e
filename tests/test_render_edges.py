"""Edges of the point-cloud renderer: the fp32 twin (oracle/render_oracle_np.py: point_fragments + scatter_min) against the
float64 model of the same rule (point_fragments_f64) on hard clouds and views (tests/helpers/render_cases.py): points exactly on
each clip plane and one fp32 step either side, at the near and the far plane, with cw == 0 or < 0, on anchor ties, sprites off
each edge, equal depths, reds outside [0, 1] or NaN, NaN / inf coordinates, 65 views, 64-point boxes that touch a view only
on its plane (one view, and the outermost of three), depths whose fp32 zw is exact.  Then (GPU) every point path of the product byte for byte against the twin on every family.

The float64 criterion, per point.  Each fp32 clip coordinate c_r is a 4-term sum of rounded products, so
|c_r(fp32) - c_r| <= E_r = 3u * T_r, T_r = sum_j |m_rj p_j| + |m_r3|, u = 2^-24 (test_bound_holds checks it).  Through the
reciprocal and the window transform, with rho = c / cw:
    |rho(fp32) - rho| <= (E_r + |rho| E_w) / cw + 2u |rho|,
    |xw(fp32) - xw| <= W (|drho| / 2 + 2u) (+ u (|xw| + 1) for the even sizes' + 0.5), zw likewise with 1 for W;
and the depth, round(zw (2^24 - 1)) in fp32 (one rounding of the product, one of the + 0.5, at spacing <= 1), may differ
from the model's by ceil(|dzw| (2^24 - 1) + 2) steps.  A point is EXEMPT when its float64 values lie within these bounds of
a decision: cw within E_w of 0, |c_r| within E_r + E_w of cw (keep), xw or yw within its bound of an anchor tie (anchor), red * 255
within 2u * 255 of k + 1/2 (colour), or its fp32 sums leave the normal range (T_r >= 2^127, cw < 2^-120: overflow, the fp32
reciprocal of a subnormal).  Elsewhere keep, anchor and colour are equal and the depth is within its bound.  Per pixel: the
twin's keys equal the min-scatter of the model's fragments with, for exempt points only, the twin's keep / anchor / colour,
and every depth the twin's where it is within its bound (so a depth outside its bound -- the far plane wrapping to 0 --
fails here too).
"""
import numpy as np
import pytest

from helpers import render_cases as rc
from oracle import render_oracle_np as ro

try:
    import torch
except ImportError:  # the CPU tier does not need it
    torch = None

f32 = np.float32
U = 2.0 ** -24
D = float(ro.DEPTH_MAX)
CPU_SIZES = [(64, 48), (320, 240), (150, 90)]
# Points built on a decision boundary (a case's bulk mask is False for them) are exempt by construction -- keep / anchor
# only; depth and colour are still checked.  Among every family's other points the exempt share must stay below BULK_EXEMPT.
# Two families have no such points: every point of theirs is on a clip plane / an anchor tie or one fp32 step off it.
BULK_EXEMPT = 0.02
ALL_ON_BOUNDARIES = {"clip_planes", "ties"}


def model_bounds(xyz, m, W, H, size):
    """-> dict of float64 clip / window values of the model and their derived fp32 error bounds, per point."""
    M = np.asarray(m, f32).astype(np.float64).reshape(4, 4).T
    P = np.asarray(xyz, f32).astype(np.float64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        c = P @ M[:, :3].T + M[:, 3]
        T = np.abs(P) @ np.abs(M[:, :3]).T + np.abs(M[:, 3])
        E = 3 * U * T * (1 + 1e-6)
        cx, cy, cz, cw = c.T
        Ex, Ey, Ez, Ew = E.T
        in_range = np.isfinite(T).all(1) & (T < 2.0 ** 127).all(1) & (np.abs(cw) >= 2.0 ** -120) & np.isfinite(c).all(1)
        keep_ex = (np.abs(cw) <= Ew) | (np.abs(cw - np.abs(cx)) <= Ex + Ew) | (np.abs(cw - np.abs(cy)) <= Ey + Ew) | \
            (np.abs(cw - np.abs(cz)) <= Ez + Ew)
        rho = c[:, :3] / cw[:, None]
        drho = (E[:, :3] + np.abs(rho) * Ew[:, None]) / np.abs(cw[:, None]) + 2 * U * np.abs(rho)
        xw, yw, zw = (rho[:, 0] * 0.5 + 0.5) * W, (rho[:, 1] * 0.5 + 0.5) * H, rho[:, 2] * 0.5 + 0.5
        exw = W * (drho[:, 0] / 2 + 2 * U) + U * (np.abs(xw) + 1)
        eyw = H * (drho[:, 1] / 2 + 2 * U) + U * (np.abs(yw) + 1)
        ezw = drho[:, 2] / 2 + 2 * U
        off = 0.0 if size & 1 else 0.5
        dtie = lambda v: np.abs((v + off) - np.rint(v + off))   # distance to the anchor's decision (floor(v + off) changes)
        kept = (cw > 0) & (np.abs(c[:, :3]) <= cw[:, None]).all(1)
        anchor_ex = kept & ((dtie(xw) <= exw) | (dtie(yw) <= eyw))   # (the anchor of a clipped point decides nothing)
        derr = np.ceil(ezw * D + 2)
    return dict(c=c, E=E, xw=xw, yw=yw, zw=zw, exw=exw, eyw=eyw, ezw=ezw, derr=derr,
                exempt=~in_range | keep_ex | anchor_ex, in_range=in_range)


def colour_exempt(red):
    r = np.asarray(red, f32).astype(np.float64)
    with np.errstate(invalid="ignore"):
        v = np.clip(r, 0, 1) * 255
        return np.abs(v - np.floor(v) - 0.5) <= 2 * U * 255


def compare_points(case, m, W, H):
    """Per-point criterion for one view -> (number of exempt points among the case's bulk points, number of bulk points)."""
    size = ro.point_size_rule(case["point_size"])
    xyz, red = case["xyz"], case["red"]
    t = ro.point_fragments(xyz, red, m, W, H, size)
    f = ro.point_fragments_f64(xyz, red, m, W, H, size)
    b = model_bounds(xyz, m, W, H, size)
    ex = b["exempt"]
    kT, kM = t[0], f[0]
    assert (kT[~ex] == kM[~ex]).all(), f"keep differs at {np.flatnonzero((kT != kM) & ~ex)[:5]}"
    both = kT & kM & ~ex
    for i, name in ((1, "x0"), (2, "y0")):
        assert (t[i][both] == f[i][both]).all(), f"{name} differs at {np.flatnonzero(both & (t[i] != f[i]))[:5]}"
    kk = kT & kM
    cex = colour_exempt(red)
    assert (t[4][kk & ~cex] == f[4][kk & ~cex]).all(), "colour differs"
    dd = np.abs(t[3].astype(np.int64) - f[3].astype(np.int64))
    bad = kk & (dd > b["derr"])
    assert not bad.any(), f"depth differs beyond its bound at {np.flatnonzero(bad)[:5]}: twin {t[3][bad][:5]} model {f[3][bad][:5]}"
    bulk = case.get("bulk", np.ones(len(ex), bool))
    return int((ex & bulk).sum()), int(bulk.sum())


def reconciled_keys(case, m, W, H):
    """The model's fragments with the twin's keep / anchor / colour for exempt points and the twin's depth where within its
    bound, min-scattered."""
    size = ro.point_size_rule(case["point_size"])
    xyz, red = case["xyz"], case["red"]
    t = ro.point_fragments(xyz, red, m, W, H, size)
    f = ro.point_fragments_f64(xyz, red, m, W, H, size)
    b = model_bounds(xyz, m, W, H, size)
    ex = b["exempt"]
    keep = np.where(ex, t[0], f[0])
    x0, y0 = np.where(ex, t[1], f[1]), np.where(ex, t[2], f[2])
    close = np.abs(t[3].astype(np.int64) - f[3].astype(np.int64)) <= b["derr"]
    depth = np.where(close | (ex & ~f[0]), t[3], f[3])
    colour = np.where(colour_exempt(red) | (ex & ~f[0]), t[4], f[4])
    return ro.scatter_min(keep, x0, y0, depth, colour, W, H, size)


def all_cases(W, H):
    return [(fam, i, c) for fam, lst in rc.families(W, H).items() for i, c in enumerate(lst)]


# ----------------------------------------------------------------------------------------------------- CPU tier
@pytest.mark.parametrize("shape", CPU_SIZES, ids=[f"{w}x{h}" for w, h in CPU_SIZES])
def test_families_reach_their_branches(shape):
    W, H = shape
    fams = rc.families(W, H)
    assert set(fams) == set(rc.EXPECTED_BRANCHES)
    for fam, lst in fams.items():
        seen = rc.reached(lst, W, H)
        missing = rc.EXPECTED_BRANCHES[fam] - seen
        assert not missing, f"{W}x{H} {fam}: does not reach {missing}"
        print(f"{W}x{H} {fam}: {sorted(seen)}")


@pytest.mark.parametrize("family", list(rc.EXPECTED_BRANCHES))
@pytest.mark.parametrize("shape", CPU_SIZES, ids=[f"{w}x{h}" for w, h in CPU_SIZES])
def test_twin_meets_float64_model_per_point(family, shape):
    W, H = shape
    n_ex = n = 0
    for c in rc.families(W, H)[family]:
        for m in c["mvps"]:
            e, k = compare_points(c, m, W, H)
            n_ex, n = n_ex + e, n + k
    assert (n == 0) == (family in ALL_ON_BOUNDARIES), (family, n)
    assert n_ex <= BULK_EXEMPT * n, f"{family}: {n_ex} of {n} points off the boundaries exempt"


@pytest.mark.parametrize("family", list(rc.EXPECTED_BRANCHES))
def test_twin_meets_float64_model_per_pixel(family):
    W, H = 150, 90
    for i, c in enumerate(rc.families(W, H)[family]):
        size = ro.point_size_rule(c["point_size"])
        for s, m in enumerate(c["mvps"]):
            got = ro.scatter_min(*ro.point_fragments(c["xyz"], c["red"], m, W, H, size), W, H, size)
            exp = reconciled_keys(c, m, W, H)
            assert (got == exp).all(), f"{family}[{i}] view {s}: {(got != exp).sum()} pixels differ"


@pytest.mark.filterwarnings("ignore::RuntimeWarning")
def test_bound_holds():
    """The derived fp32 error bounds hold on every family: clip coordinates within E_r, window coordinates within their bounds
    (points the model and the twin both keep), depth within derr (compare_points)."""
    for W, H in CPU_SIZES:
        for fam, i, c in all_cases(W, H):
            size = ro.point_size_rule(c["point_size"])
            for m in c["mvps"]:
                b = model_bounds(c["xyz"], m, W, H, size)
                ok = b["in_range"]
                c32 = np.stack(ro.clip_fp32(c["xyz"], m), 1).astype(np.float64)
                assert (np.abs(c32 - b["c"])[ok] <= b["E"][ok]).all(), (W, H, fam, i)
                keep = ro.point_fragments(c["xyz"], c["red"], m, W, H, size)[0] & ro.point_fragments_f64(c["xyz"], c["red"], m, W, H, size)[0] & ok
                xw, yw, zw = (v.astype(np.float64) for v in ro.window_fp32(c["xyz"], m, W, H))
                assert (np.abs(xw - b["xw"])[keep] <= b["exw"][keep]).all(), (W, H, fam, i, "xw")
                assert (np.abs(yw - b["yw"])[keep] <= b["eyw"][keep]).all(), (W, H, fam, i, "yw")
                assert (np.abs(zw - b["zw"])[keep] <= b["ezw"][keep]).all(), (W, H, fam, i, "zw")


@pytest.mark.parametrize("shape", CPU_SIZES, ids=[f"{w}x{h}" for w, h in CPU_SIZES])
def test_depth_rounding_is_exact_where_zw_is(shape):
    """The depth is round-half-up of zw (2^24 - 1), not truncation: where the fp32 zw is exact (the exact_depth family: the
    twin's zw equals the model's), the only fp32 roundings left are those of the product and of the + 0.5, each at most half a
    spacing (the second none where the spacing is at most 1/2); farther than that from the rounding decision the twin's depth must equal the model's exactly.  The family puts
    every point there, half of them rounding up."""
    W, H = shape
    c = rc.families(W, H)["exact_depth"][0]
    m = c["mvps"][0]
    t = ro.point_fragments(c["xyz"], c["red"], m, W, H, 1)
    f = ro.point_fragments_f64(c["xyz"], c["red"], m, W, H, 1)
    assert t[0].all() and f[0].all()
    zw32 = ro.window_fp32(c["xyz"], m, W, H)[2].astype(np.float64)
    assert (zw32 == model_bounds(c["xyz"], m, W, H, 1)["zw"]).all()
    v = zw32 * D
    sp = np.spacing(v.astype(f32)).astype(np.float64)
    e = sp / 2 + np.where(sp <= 0.5, 0.0, sp / 2)   # (a product on a grid of spacing <= 1/2 takes the + 0.5 exactly)
    decided = np.abs(v - np.floor(v) - 0.5) > e
    assert decided.all()
    assert (t[3] == f[3]).all(), f"{(t[3] != f[3]).sum()} depths differ"
    up = f[3] > v
    assert 0.3 < up.mean() < 0.7


def test_exemption_is_rare_on_an_ordinary_cloud():
    from test_render import plane_cloud
    W, H = 160, 120
    xyz, red, _ = plane_cloud(W, H)
    rng = np.random.default_rng(5)
    xyz = np.concatenate([xyz, rng.uniform(-30, 30, (5000, 3)).astype(f32)])
    red = np.concatenate([red, rng.uniform(-0.2, 1.2, 5000).astype(f32)])
    case = {"xyz": xyz, "red": red, "point_size": 3.0}
    m = rc.cameras(W, H)["oblique"]
    n_ex, n = compare_points(case, m, W, H)
    assert n_ex < 0.005 * n, (n_ex, n)
    assert (ro.render_keys(xyz, red, m, W, H, 3.0) == reconciled_keys(case, m, W, H)).all()


def test_far_plane_point_has_the_largest_depth_and_loses():
    W, H = 64, 48
    m = rc.cameras(W, H)["axis"]
    far = np.array([[0, 0, rc.ZF]], f32)
    keep, x0, y0, depth, colour = ro.point_fragments(far, np.array([0.2], f32), m, W, H, 3)
    assert keep[0] and depth[0] == ro.DEPTH_MAX
    assert ro.point_fragments_f64(far, np.array([0.2], f32), m, W, H, 3)[3][0] == ro.DEPTH_MAX
    two = np.array([[0, 0, rc.ZF], [0, 0, 10.0]], f32)
    for order in ([0, 1], [1, 0]):
        img = ro.render_points(two[order], np.array([0.1, 0.9], f32)[order], m, W, H, 1)
        assert img[H // 2, W // 2] == round(0.9 * 255)   # the nearer point wins in either draw order
    # 1e-7 relative inside the far plane: the largest depth too, or one below
    inside = np.array([[0, 0, rc.ZF * (1 - 1e-7)]], f32)
    assert ro.point_fragments(inside, np.array([0.2], f32), m, W, H, 3)[3][0] >= ro.DEPTH_MAX - 1


def test_far_plane_white_point_is_the_empty_key():
    """depth 2^24 - 1 with colour 255 is 0xFFFFFFFF: the pixel shows 255 and is not covered (nmi_render_points_masked)."""
    W, H = 64, 48
    m = rc.cameras(W, H)["axis"]
    p = np.array([[0, 0, rc.ZF]], f32)
    assert (ro.coverage(p, np.array([1.0], f32), m, W, H, 1) == 0).all()
    assert ro.coverage(p, np.array([0.99], f32), m, W, H, 1).sum() == 1


@pytest.mark.parametrize("ps,size", [(0.0, 1), (0.49, 1), (0.5, 1), (1.49, 1), (1.5, 2), (4.5, 5), (63.5, 64), (64.4, 64),
                                     (1e10, 64), (np.inf, 64), (-np.inf, 1), (-1e10, 1), (-3.0, 1)])
def test_point_size_rule(ps, size):
    assert ro.point_size_rule(ps) == size


def test_point_size_rule_rejects_nan():
    with pytest.raises(ValueError):
        ro.point_size_rule(np.nan)


def test_twin_nan_clip_coordinate_is_dropped():
    """cx = inf - inf (NaN) with cy, cz, cw inside: the twin drops the point; the float64 model, which does not overflow, keeps it
    (an fp32 range exemption)."""
    c = rc.families(64, 48)["nonfinite"][1]
    keep = ro.point_fragments(c["xyz"], c["red"], c["mvps"][0], 64, 48, 1)[0]
    cx = ro.clip_fp32(c["xyz"], c["mvps"][0])[0]
    assert np.isnan(cx).sum() >= 2 and not keep[np.isnan(cx)].any() and keep[~np.isnan(cx)].any()


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


def twin_stack(c, W, H, mvps=None):
    mvps = c["mvps"] if mvps is None else mvps
    keys = np.stack([ro.render_keys(c["xyz"], c["red"], m, W, H, c["point_size"]) for m in mvps]).reshape(len(mvps), H, W)
    return (keys & np.uint32(0xFF)).astype(np.uint8), (keys != ro.EMPTY).astype(np.uint8)


def views_differ(name, got, exp):
    return [f"{name} view {s}: {(got[s] != exp[s]).sum()} px" for s in range(len(exp)) if not (got[s] == exp[s]).all()]


# 160 x 120: the fast resolves (sizes <= 5, width % 4 == 0); 150 x 90: the any-size resolves for every size
GPU_SIZES = [(160, 120), (150, 90)]


@pytest.mark.gpu
@pytest.mark.parametrize("family", list(rc.EXPECTED_BRANCHES))
@pytest.mark.parametrize("shape", GPU_SIZES, ids=[f"{w}x{h}" for w, h in GPU_SIZES])
def test_gpu_render_points_families(nmi, family, shape):
    """nmi_render_points and nmi_render_points_masked (both resolves of each) byte for byte against the twin, the masks against
    the twin's coverage; and the same renders after nmi_sort_points (the depth test is a minimum: order-free)."""
    W, H = shape
    cases = rc.families(W, H)[family]
    assert rc.EXPECTED_BRANCHES[family] <= rc.reached(cases, W, H)
    bad = []
    with nmi.NmiContext(W, H) as ctx:
        for i, c in enumerate(cases):
            exp, cov = twin_stack(c, W, H)
            dx, dr = dev(c["xyz"]), dev(c["red"])
            got = ctx.render_points(dx, dr, c["mvps"], c["point_size"]).cpu().numpy()
            bad += views_differ(f"{family}[{i}] render", got, exp)
            r2, m2 = ctx.render_points_masked(dx, dr, c["mvps"], c["point_size"])
            bad += views_differ(f"{family}[{i}] masked render", r2.cpu().numpy(), exp)
            bad += views_differ(f"{family}[{i}] mask", m2.cpu().numpy(), cov)
            sx, sr = ctx.sort_points(dx, dr)
            bad += views_differ(f"{family}[{i}] sorted", ctx.render_points(sx, sr, c["mvps"], c["point_size"]).cpu().numpy(), exp)
    assert not bad, bad[:10]


def _replays(c):
    """A level's parameters replay after replay: the case's views, every view moved by a small world translation, the case's
    views again (whatever the second replay culled, listed or splatted must not linger)."""
    m2 = rc.shifted(c["mvps"], (0.07, -0.05, 0.3))
    assert all(not np.array_equal(a, b) for a, b in zip(c["mvps"], m2)), "a replay's view did not change"
    return [c["mvps"], m2, c["mvps"]]


@pytest.mark.gpu
@pytest.mark.parametrize("family", list(rc.EXPECTED_BRANCHES))
@pytest.mark.parametrize("shape", [(320, 240), (150, 90)], ids=["320x240-fused", "150x90"])
def test_gpu_level_families(nmi, family, shape):
    """A point-cloud NmiLevel (prep with the common-plane cull of the packed cloud's boxes, the front kernel's splat, the
    resolve) and a covered one (nmi_zbuf_resolve_fast_kernel's coverage form with the epoch) against the twin, over three replays with changing
    matrices."""
    W, H = shape
    bad = []
    with nmi.NmiContext(W, H) as ctx:
        frame = dev(np.random.default_rng(0).integers(0, 256, (H, W), dtype=np.uint8))
        for i, c in enumerate(rc.families(W, H)[family]):
            dx, dr = dev(c["xyz"]), dev(c["red"])
            S = len(c["mvps"])
            for covered in (False, True):
                with nmi.NmiLevel(ctx, dx, dr, frame, S, 1, c["point_size"]) as lv:
                    if covered:
                        lv.set_coverage(True)
                    for rep, mv in enumerate(_replays(c)):
                        lv.run(mv, np.eye(3)[None])
                        exp, cov = twin_stack(c, W, H, mv)
                        tag = f"{family}[{i}] {'covered ' if covered else ''}level replay {rep}"
                        bad += views_differ(tag, lv.outputs()[0], exp)
                        if covered:
                            bad += views_differ(tag + " coverage", lv.coverage()[0], cov)
    assert not bad, bad[:10]


@pytest.mark.gpu
def test_gpu_point_size_rule(nmi):
    """1e10 and inf render as 64 (not as 1), NaN is rejected by nmi_render_points, nmi_render_points_masked and
    nmi_level_create; the context stays usable."""
    from orbslam2_nmi_amd import capi
    W, H = 150, 90
    c = rc.families(W, H)["edges"][0]
    dx, dr = dev(c["xyz"]), dev(c["red"])
    with nmi.NmiContext(W, H) as ctx:
        ref = ctx.render_points(dx, dr, c["mvps"], 64.0).cpu().numpy()
        for ps in (64.4, 1e10, np.inf):
            assert (ctx.render_points(dx, dr, c["mvps"], ps).cpu().numpy() == ref).all(), ps
        assert (ctx.render_points(dx, dr, c["mvps"], -np.inf).cpu().numpy() == ctx.render_points(dx, dr, c["mvps"], 1.0).cpu().numpy()).all()
        for call in (lambda: ctx.render_points(dx, dr, c["mvps"], np.nan), lambda: ctx.render_points_masked(dx, dr, c["mvps"], np.nan),
                     lambda: nmi.NmiLevel(ctx, dx, dr, dev(np.zeros((H, W), np.uint8)), len(c["mvps"]), 1, np.nan)):
            with pytest.raises(capi.NmiError) as e:
                call()
            assert e.value.code == capi.ERR_INVALID_ARGUMENT
        assert (ctx.render_points(dx, dr, c["mvps"], 64.0).cpu().numpy() == ref).all()


# ---------------------------------------------------------------------------------------------- the mesh path's far plane
def _far_and_near_mesh(W, H):
    from test_render import plane_mesh
    n = 3 * 2 * 4 * 3
    xf, uf, rgb, rp = plane_mesh(W, H, depth=rc.ZF, nx=4, ny=3)        # exactly at the far plane (params(): far = 30)
    xn, un, _, _ = plane_mesh(W, H, depth=10.0, nx=4, ny=3)
    xn = xn[:n] * np.float32([0.5, 0.5, 1])                               # a smaller plane, nearer, in the middle of the view
    return xf[:n], uf[:n], xn, (un[:n] + np.float32(0.31)).astype(f32), rgb, rp


def test_mesh_twin_far_plane_has_the_largest_depth_and_loses():
    """The mesh renderer already clamps: a triangle at z = 1 gets depth 0xFFFFFF and loses to nearer geometry in either draw
    order -- the rule the point renderer now shares."""
    from oracle import mesh_oracle_np as mo
    W, H = 96, 72
    xf, uf, xn, un, rgb, rp = _far_and_near_mesh(W, H)
    lv = mo.mip_luma(rgb)
    m = rc.cameras(W, H)["axis"]
    zbuf = np.full((H, W), 0xFFFFFFFFFF, np.uint64)
    P, T = xf.reshape(-1, 3, 3), uf.reshape(-1, 3, 2)
    for t in range(len(P)):
        c = ro.clip_fp32(P[t], m)
        for sub in mo._clip_near(*c, T[t, :, 0], T[t, :, 1]):
            mo._raster(zbuf, lv, W, H, *sub)
    drawn = zbuf != 0xFFFFFFFFFF
    d = zbuf[drawn] >> np.uint64(8)
    # (the interpolated z is 1 or a few fp32 steps either side of it; above 1 the fragment is depth-clipped)
    assert drawn.mean() > 0.5 and (d >= 0xFFFFF0).all() and (d <= 0xFFFFFF).all() and (d == 0xFFFFFF).mean() > 0.5
    near = mo.render_mesh(xn, un, lv, m, W, H)
    inner = near != 255
    assert inner.mean() > 0.1
    for xyz, uv in ((np.concatenate([xf, xn]), np.concatenate([uf, un])), (np.concatenate([xn, xf]), np.concatenate([un, uf]))):
        img = mo.render_mesh(xyz, uv, lv, m, W, H)
        assert (img[inner] == near[inner]).all()


@pytest.mark.gpu
def test_gpu_mesh_far_plane_loses_to_nearer_geometry(nmi):
    from oracle import mesh_oracle_np as mo
    W, H = 96, 72
    xf, uf, xn, un, rgb, rp = _far_and_near_mesh(W, H)
    lv = mo.mip_luma(rgb)
    m = rc.cameras(W, H)["axis"]
    with nmi.NmiContext(W, H) as ctx:
        tex = nmi.NmiTexture(ctx, rgb)
        for xyz, uv in ((np.concatenate([xf, xn]), np.concatenate([uf, un])), (np.concatenate([xn, xf]), np.concatenate([un, uf]))):
            got = ctx.render_mesh(dev(xyz), dev(uv), tex, m[None]).cpu().numpy()[0]
            assert (got == mo.render_mesh(xyz, uv, lv, m, W, H)).all()
