"""Hard point clouds, views and sizes for the point-cloud renderer -- TEST INFRASTRUCTURE ONLY.

families(W, H) -> {name: [case, ...]}: the cases each family is made of for a W x H frame; a case is a dict with xyz [N, 3]
and red [N] float32, mvps [S, 16] float32 (column-major, glm layout) and point_size.
branches(case, W, H) -> the names of the branches of the point rule that the case reaches, computed from the fp32 twin's
per-point arrays (oracle/render_oracle_np.py).
EXPECTED_BRANCHES: the branches a family exists to reach (on frames of at least 64 x 48); a family that quietly stops reaching
them makes its tests fail instead of passing vacuously.

Points on a decision boundary are found in fp32, not guessed: fp32_root walks one coordinate of a point over adjacent floats
until the twin's fp32 expression (c - cw, xw - k, ...) is exactly zero, and the families keep those points and their
one-step neighbours.  Matrices are Projection * lookAt in float64 (ro.projection, ro.look_at), rounded to fp32, or written
directly.
"""
import numpy as np

from oracle import render_oracle_np as ro
from orbslam2_nmi_amd import synthetic as sy

f32 = np.float32
D_MAX = float(ro.DEPTH_MAX)
ZN, ZF = 5.0, 30.0
SIZES = (1, 2, 3, 7, 8, 64)
POINT_SIZES = (0.49, 0.5, 4.5, 64.4, 1e10, np.inf)


def mvp(W, H, eye, look, up, zn=ZN, zf=ZF):
    K = sy.intrinsics(W, H)
    M = ro.projection(K[0, 0], K[1, 1], K[0, 2], K[1, 2], zn, zf) @ ro.look_at(eye, look, up)
    return M.T.reshape(16).astype(f32)   # column-major


def cameras(W, H):
    """axis-aligned, rolled, pitched, and yawed + rolled + pitched (all at the origin, looking along about +z)."""
    r = np.radians
    return {
        "axis": mvp(W, H, (0, 0, 0), (0, 0, 1), (0, -1, 0)),
        "rolled": mvp(W, H, (0, 0, 0), (0, 0, 1), (np.sin(r(30)), -np.cos(r(30)), 0)),
        "pitched": mvp(W, H, (0, 0, 0), (0, np.sin(r(20)), np.cos(r(20))), (0, -np.cos(r(20)), np.sin(r(20)))),
        "oblique": mvp(W, H, (0.3, -0.2, 0.1), (0.3 + np.sin(r(15)), -0.2 + 0.2, 0.1 + np.cos(r(15))), (np.sin(r(-25)), -np.cos(r(-25)), 0)),
    }


def unproject(m, W, H, xw, yw, zw):
    """float64 world points whose float64 window coordinates under the fp32 matrix m are (xw, yw, zw)."""
    M = np.asarray(m, f32).astype(np.float64).reshape(4, 4).T
    ndc = np.stack([2 * np.asarray(xw, float) / W - 1, 2 * np.asarray(yw, float) / H - 1, 2 * np.asarray(zw, float) - 1,
                    np.ones(np.broadcast(xw, yw, zw).shape)], -1)
    X = ndc @ np.linalg.inv(M).T
    return X[..., :3] / X[..., 3:]


def _ordered(x):
    b = np.asarray(x, f32).view(np.int32).astype(np.int64)
    return np.where(b < 0, -(b & 0x7FFFFFFF), b)


def _unordered(o):
    o = np.asarray(o, np.int64)
    return np.where(o < 0, (-o) | 0x80000000, o).astype(np.uint32).view(f32)


def fp32_root(fun, P, k, reach=1e-3):
    """Walk coordinate k of the float64 points P (each near a sign change of fun) over fp32 values: bisection on adjacent
    floats within reach * (|P_k| + 1).  fun(xyz float32 [n, 3], rows [n]) -> float64 [n], the exact difference of two fp32
    values for the points P[rows].  -> (exact [M, 3]: points where fun is exactly 0, below, above: their one-step neighbours
    along k), float32."""
    P = np.asarray(P, np.float64)
    d = reach * (np.abs(P[:, k]) + 1)
    lo, hi = P.copy(), P.copy()
    lo[:, k] -= d
    hi[:, k] += d
    lo, hi = lo.astype(f32), hi.astype(f32)
    rows = np.arange(len(P))
    with np.errstate(all="ignore"):
        flo = np.sign(fun(lo, rows))
        ok = flo * np.sign(fun(hi, rows)) < 0
        lo, hi, flo, rows = lo[ok], hi[ok], flo[ok], rows[ok]
        a, b = _ordered(lo[:, k]), _ordered(hi[:, k])
        for _ in range(40):
            mid = (a + b) // 2
            X = lo.copy()
            X[:, k] = _unordered(mid)
            left = np.sign(fun(X, rows)) == flo
            a, b = np.where(left, mid, a), np.where(left, b, mid)
        pts, o = [], []
        for cand in (a, b):
            X = lo.copy()
            X[:, k] = _unordered(cand)
            z = fun(X, rows) == 0
            pts.append(X[z])
            o.append(cand[z])
    pts, o = np.concatenate(pts), np.concatenate(o)
    below, above = pts.copy(), pts.copy()
    below[:, k], above[:, k] = _unordered(o - 1), _unordered(o + 1)
    return pts, below, above


def plane_points(m, W, H, plane, n=48, seed=0):
    """Points exactly on clip plane `plane` = (row j in 0..2, sign +-1): fp32 sign * c_j == cw, with their neighbours."""
    j, sgn = plane
    rng = np.random.default_rng(seed + 7 * j + (sgn > 0))
    t = rng.uniform(0.05, 0.95, (n, 3))
    t[:, j] = 1.0 if sgn > 0 else 0.0
    P = unproject(m, W, H, t[:, 0] * W, t[:, 1] * H, t[:, 2])

    def fun(X, rows):
        c = ro.clip_fp32(X, m)
        return sgn * c[j].astype(np.float64) - c[3].astype(np.float64)
    M = np.asarray(m, f32).astype(np.float64).reshape(4, 4).T
    k = int(np.argmax(np.abs(sgn * M[j, :3] - M[3, :3])))   # the coordinate the plane function depends on most
    return fp32_root(fun, P, k)


def tie_points(m, W, H, size, n=48, seed=1):
    """Points whose fp32 window coordinate lies exactly on an anchor tie (integers for odd sizes, half-integers for even),
    on both axes, with their neighbours."""
    rng = np.random.default_rng(seed + size)
    off = 0.0 if size & 1 else 0.5
    out = []
    for axis, ext in ((0, W), (1, H)):
        target = rng.integers(1, max(2, ext - 1), n) + off
        other = rng.uniform(0.1, 0.9, n) * (H if axis == 0 else W)
        xw, yw = (target, other) if axis == 0 else (other, target)
        P = unproject(m, W, H, xw, yw, rng.uniform(0.2, 0.8, n))
        fun = lambda X, rows, axis=axis, target=target: ro.window_fp32(X, m, W, H)[axis].astype(np.float64) - target[rows]
        M = np.asarray(m, f32).astype(np.float64).reshape(4, 4).T
        k = int(np.argmax(np.abs(M[axis, :3])))
        out += list(fp32_root(fun, P, k))
    return np.concatenate(out)


def _case(xyz, red, mvps, point_size, bulk=True):
    """bulk: [N] bool (or one bool for all): the points NOT built on a decision boundary.  The CPU tests require that almost none
    of them fall inside the twin-vs-model exemption, so that the exemption cannot swallow a family."""
    xyz = np.asarray(xyz, f32).reshape(-1, 3)
    red = np.broadcast_to(np.asarray(red, f32), (len(xyz),)).copy()
    bulk = np.broadcast_to(np.asarray(bulk, bool), (len(xyz),)).copy()
    return {"xyz": np.ascontiguousarray(xyz), "red": red, "mvps": np.asarray(mvps, f32).reshape(-1, 16), "point_size": point_size,
            "bulk": bulk}


def shifted(mvps, t):
    """The views moved: M' = M T(t) (a world translation by t), in float64, rounded to fp32."""
    out = []
    for m in np.asarray(mvps, f32).reshape(-1, 16):
        M = m.astype(np.float64).reshape(4, 4).T
        T = np.eye(4)
        T[:3, 3] = t
        out.append((M @ T).T.reshape(16).astype(f32))
    return np.stack(out)


def _reds(n, seed):
    return np.random.default_rng(seed).uniform(0.02, 0.98, n).astype(f32)


def _grid(m, W, H, zw, nx=12, ny=9):
    u, v = np.meshgrid((np.arange(nx) + 0.37) / nx * W, (np.arange(ny) + 0.61) / ny * H)
    return unproject(m, W, H, u.ravel(), v.ravel(), np.full(u.size, zw))


def families(W, H):
    cams = cameras(W, H)
    axis = cams["axis"]
    fam = {}
    # ---- every clip plane, exactly and one fp32 step either side, under an axis-aligned and an oblique camera
    cases = []
    for cname in ("axis", "oblique"):
        m = cams[cname]
        pts = [np.concatenate(plane_points(m, W, H, (j, s))) for j in range(3) for s in (-1, 1)]
        xyz = np.concatenate(pts)
        cases.append(_case(xyz, _reds(len(xyz), 1), m[None], 3.0, bulk=False))   # (every point is on a plane or a step off it)
    fam["clip_planes"] = cases
    # ---- the far and the near plane exactly, under axis-aligned, rolled and pitched cameras; a far-plane grid (z = far, which
    # rounds to zw = 1) over a nearer one of the same pixels, in both draw orders: the far points must lose
    cases = []
    for cname in ("axis", "rolled", "pitched"):
        m = cams[cname]
        xyz = np.concatenate([np.concatenate(plane_points(m, W, H, (2, s), seed=5)) for s in (-1, 1)])
        cases.append(_case(xyz, _reds(len(xyz), 2), m[None], 3.0, bulk=False))
    far = _grid(axis, W, H, 0.5)
    far[:, 2] = ZF
    near = far.copy()
    near[:, 2] = 10.0
    near[:, :2] *= 10.0 / ZF
    for order in (0, 1):
        xyz = np.concatenate([far, near] if order == 0 else [near, far])
        red = np.concatenate([np.full(len(far), 0.1), np.full(len(near), 0.9)] if order == 0 else
                             [np.full(len(near), 0.9), np.full(len(far), 0.1)])
        bulk = np.r_[np.zeros(len(far), bool), np.ones(len(near), bool)]   # the nearer grid is on no boundary
        cases.append(_case(xyz, red, axis[None], 3.0, bulk=bulk if order == 0 else bulk[::-1]))
    cases.append(_case(far, np.linspace(0, 1, len(far)), axis[None], 2.0, bulk=False))   # alone: colour 255 at the far plane = the empty key
    fam["near_far"] = cases
    # ---- cw == 0 (points in the camera's plane), cw < 0, behind the camera, cw one step above 0
    rng = np.random.default_rng(3)
    xy = rng.uniform(-5, 5, (40, 2))
    pts = [np.c_[xy, np.zeros(40)], np.c_[xy, -rng.uniform(0.1, 40, 40)], np.c_[xy * 1e-30, np.full(40, 1e-30)],
           np.c_[np.zeros((4, 2)), [1e-38, 1e-40, 1e-44, 1e-45]]]
    xyz = np.concatenate(pts)
    bulk = np.r_[np.zeros(40, bool), np.ones(40, bool), np.zeros(44, bool)]   # (cw < 0 by far more than its error: no boundary)
    cases = [_case(xyz, _reds(len(xyz), 3), np.stack([cams[c] for c in ("axis", "rolled", "oblique")]), 3.0, bulk=bulk)]
    crafted = np.zeros(16, f32)   # cx = x, cy = y, cz = 0, cw = z: subnormal and tiny cw with the point inside the planes
    crafted[0], crafted[5], crafted[11] = 1, 1, 1
    cases.append(_case(np.c_[np.zeros((6, 2)), [1e-30, 1e-37, 1e-38, 1e-39, 1e-44, 0.0]], 0.5, crafted[None], 1.0, bulk=False))
    fam["behind"] = cases
    # ---- anchor ties: integers for odd sizes, half-integers for even sizes
    fam["ties"] = [_case(tie_points(cams[c], W, H, s), _reds(1, 4)[0], cams[c][None], float(s), bulk=False)
                   for c, s in (("axis", 1), ("axis", 2), ("oblique", 3), ("rolled", 8))]
    # ---- sprites hanging off each edge, for every size and the odd point sizes
    t = np.linspace(0.05, 0.95, 7) + 0.0123   # (off the anchor ties: those are the "ties" family's)
    e = [0.0113, 0.5071, 0.9913]
    win = [(x, y) for x in e for y in t] + [(x, y) for y in e for x in t]
    u = np.array([w[0] for w in win]) * W
    v = np.array([w[1] for w in win]) * H
    u = np.concatenate([u, [0.013, W - 2e-3, 0.2, W - 0.2]])
    v = np.concatenate([v, [0.2, H - 0.2, 0.013, H - 2e-3]])
    xyz = unproject(axis, W, H, u, v, np.linspace(0.1, 0.9, len(u)))
    fam["edges"] = [_case(xyz, _reds(len(xyz), 5), np.stack([axis, cams["rolled"]]), float(s)) for s in SIZES] + \
                   [_case(xyz, _reds(len(xyz), 6), axis[None], ps) for ps in POINT_SIZES]
    # ---- equal quantised depths with different reds: the same point several times, and neighbours along a view ray
    base = _grid(axis, W, H, 0.6, 5, 4)
    xyz = np.concatenate([base, base, base, base * np.float32(1 + 2 ** -23)])
    red = np.concatenate([np.full(len(base), 0.7), np.full(len(base), 0.2), np.full(len(base), 0.45), np.full(len(base), 0.6)])
    fam["equal_depth"] = [_case(xyz, red, axis[None], 3.0), _case(xyz[::-1], red[::-1], axis[None], 2.0)]
    # ---- reds outside [0, 1], NaN and infinite
    xyz = _grid(axis, W, H, 0.4, 6, 3)
    red = np.resize(np.array([-1, 1.5, np.nan, np.inf, -np.inf, 0.5], f32), len(xyz))
    fam["reds"] = [_case(xyz, red, axis[None], 3.0), _case(np.concatenate([xyz, xyz]), np.concatenate([red, red[::-1]]), axis[None], 1.0)]
    # ---- NaN and infinite coordinates; near-FLT_MAX coordinates under a matrix whose x row is inf - inf (cx NaN alone)
    good = _grid(axis, W, H, 0.5, 4, 3)
    bad = np.array([[np.nan, 0, 10], [0, np.nan, 10], [0, 0, np.nan], [np.inf, 0, 10], [-np.inf, 0, 10], [0, np.inf, 10],
                    [0, 0, np.inf], [0, 0, -np.inf], [np.inf, np.inf, np.inf]])
    xyz = np.concatenate([good, bad])
    cases = [_case(xyz, _reds(len(xyz), 7), np.stack([axis, cams["oblique"]]), 3.0, bulk=np.r_[np.ones(len(good), bool), np.zeros(len(bad), bool)])]
    nanx = np.zeros(16, f32)   # cx = 2 x - 2 y, cy = y / 4e38, cz = 0, cw = 1
    nanx[0], nanx[4], nanx[5], nanx[15] = 2, -2, 1 / 4e38, 1
    big = np.array([[3e38, 3e38, 0], [3.4e38, 3.4e38, 0], [-3e38, -3e38, 0], [1.0, 1.0, 0], [3e38, 0.5, 0], [0.25, 0.25, 0]], np.float64)
    cases.append(_case(big, [0.3, 0.4, 0.5, 0.6, 0.7, 0.8], nanx[None], 1.0, bulk=False))
    fam["nonfinite"] = cases
    # ---- S = 65 views (two launches of the splat), some looking back at the cloud from beyond it
    rng = np.random.default_rng(9)
    xyz = rng.uniform(-1, 1, (3000, 3)) * [6, 5, 8] + [0, 0, 15]
    views = []
    for s in range(65):
        if s % 5 == 4:
            views.append(mvp(W, H, (0.1 * s / 65, 0, 32), (0, 0, 15), (0, -1, 0)))   # looking back along -z
        else:
            views.append(mvp(W, H, (0.05 * (s % 7), -0.04 * (s % 3), 0.1 * (s % 4)), (0.02 * s / 65, 0, 1), (0, -1, 0)))
    fam["many_views"] = [_case(xyz, _reds(len(xyz), 8), np.stack(views), 3.0)]
    # ---- 64-point wavefront boxes outside a view except for points exactly on its plane (the per-wavefront cull)
    cases = []
    for cname in ("axis", "oblique"):
        m = cams[cname]
        chunks = []
        for j, s in ((0, 1), (0, -1), (1, 1), (1, -1)):
            on = plane_points(m, W, H, (j, s), n=16, seed=11)[0][:4]
            t = np.random.default_rng(j).uniform(0.2, 0.8, (60, 3))
            t[:, j] = 1.02 if s > 0 else -0.02   # outside the same plane
            out = unproject(m, W, H, t[:, 0] * W, t[:, 1] * H, t[:, 2])
            if len(on):
                chunks.append((out, np.concatenate([on, np.repeat(on[-1:], 64 - 60 - len(on), 0)])))
        xyz = np.concatenate([np.concatenate(c) for c in chunks])
        bulk = np.concatenate([np.r_[np.ones(len(a), bool), np.zeros(len(b), bool)] for a, b in chunks])
        cases.append(_case(xyz, _reds(len(xyz), 12), m[None], 1.0, bulk=bulk))
    # the same with three views side by side: a level bounds the union of their frusta by six common planes
    # (level_views_bound, with a margin), and the outermost view's side plane is that bound's side.  Each box's visible points
    # lie exactly on the plane of the one view that sees them; its other points are outside every view.
    views = np.stack([mvp(W, H, (dx, 0, 0), (dx, 0, 1), (0, -1, 0)) for dx in (-0.8, 0.0, 0.8)])
    chunks = []
    for v, m in enumerate(views):
        for j, s in ((0, 1), (0, -1), (1, 1), (1, -1)):
            on = plane_points(m, W, H, (j, s), n=24, seed=13)[0]
            seen_by = np.stack([ro.point_fragments(on, np.zeros(len(on), f32), o, W, H, 1)[0] for o in views])
            on = on[seen_by[v] & (seen_by.sum(0) == 1)][:4]
            t = np.random.default_rng(20 + j).uniform(0.2, 0.8, (200, 3))
            t[:, j] = 1.05 if s > 0 else -0.05
            out = unproject(m, W, H, t[:, 0] * W, t[:, 1] * H, t[:, 2]).astype(f32)
            out = out[~np.stack([ro.point_fragments(out, np.zeros(len(out), f32), o, W, H, 1)[0] for o in views]).any(0)][:60]
            if len(on) and len(out) == 60:
                chunks.append((out, np.concatenate([on, np.repeat(on[-1:], 4 - len(on), 0)])))
    xyz = np.concatenate([np.concatenate(c) for c in chunks])
    bulk = np.concatenate([np.r_[np.ones(len(a), bool), np.zeros(len(b), bool)] for a, b in chunks])
    cases.append(_case(xyz, _reds(len(xyz), 14), views, 1.0, bulk=bulk))
    fam["box_planes"] = cases
    # ---- depth rounding where the fp32 window depth is exact: cx = x, cy = y, cz = z, cw = 1 and z = a / 2^24 - 1 with
    # 2^22 < a < 2^23, so zw = a / 2^25 in (1/8, 1/4) with no rounding.  zw (2^24 - 1) = a / 2 - zw: an even a has a fraction
    # of 1 - zw (> 3/4: rounds UP -- truncation would give one less), an odd a one of 1/2 - zw (< 3/8: rounds down).  The fp32
    # product is within 1/8 of it (spacing 1/4 below 2^22) and takes the + 0.5 exactly, so fp32 and float64 agree.
    exact = np.zeros(16, f32)
    exact[0], exact[5], exact[10], exact[15] = 1, 1, 1, 1
    rng = np.random.default_rng(15)
    a = rng.integers((1 << 22) + 1, 1 << 23, 240)
    xyz = np.c_[rng.uniform(-0.9, 0.9, (len(a), 2)), a / 2.0 ** 24 - 1]
    fam["exact_depth"] = [_case(xyz, _reds(len(xyz), 16), exact[None], 1.0)]
    return fam


EXPECTED_BRANCHES = {
    "clip_planes": {"on_plane", "outside_by_step"},
    "near_far": {"far", "near", "far_behind_nearer", "empty_key"},
    "behind": {"cw_zero", "cw_negative", "cw_subnormal"},
    "ties": {"tie_odd", "tie_even"},
    "edges": {"edge_left", "edge_right", "edge_bottom", "edge_top", "size_64", "size_1"},
    "equal_depth": {"equal_depth"},
    "reds": {"red_below", "red_above", "red_nan"},
    "nonfinite": {"nan_clip", "nan_clip_alone"},
    "many_views": {"two_launches", "opposed_views"},
    "box_planes": {"box_on_plane", "box_at_common_bound"},
    "exact_depth": {"depth_round_up", "depth_round_down"},
}


def branches(case, W, H):
    """The branches of the point rule the case reaches, from the fp32 twin's per-point arrays."""
    size = ro.point_size_rule(case["point_size"])
    xyz, red, mvps = case["xyz"], case["red"], case["mvps"]
    seen = set()
    if len(mvps) > 64:
        seen.add("two_launches")
    seen.add(f"size_{size}")
    with np.errstate(all="ignore"):
        if (red < 0).any():
            seen.add("red_below")
        if (red > 1).any():
            seen.add("red_above")
        if np.isnan(red).any():
            seen.add("red_nan")
    fwd, keeps, ons = [], [], []
    for m in mvps:
        keep, x0, y0, depth, colour = ro.point_fragments(xyz, red, m, W, H, size)
        cx, cy, cz, cw = ro.clip_fp32(xyz, m)
        with np.errstate(all="ignore"):
            mag = np.maximum(np.maximum(np.abs(cx), np.abs(cy)), np.abs(cz))
            if (keep & (mag == cw)).any():
                seen.add("on_plane")
            if (~keep & (cw > 0) & (np.nextafter(cw, np.float32(np.inf)) == mag)).any():
                seen.add("outside_by_step")
            if (cw == 0).any():
                seen.add("cw_zero")
            if (cw < 0).any():
                seen.add("cw_negative")
            if ((cw > 0) & (cw < np.finfo(f32).tiny) & (mag <= cw)).any():
                seen.add("cw_subnormal")
            nanc = np.isnan(cx) | np.isnan(cy) | np.isnan(cz) | np.isnan(cw)
            if nanc.any():
                seen.add("nan_clip")
            alone = np.isnan(cx) & (np.abs(cy) <= cw) & (np.abs(cz) <= cw) & (cw > 0)
            if alone.any():
                seen.add("nan_clip_alone")
            xw, yw, _ = ro.window_fp32(xyz, m, W, H)
            tie = (xw == np.floor(xw)) | (yw == np.floor(yw)) if size & 1 else ((xw + f32(0.5)) == np.floor(xw + f32(0.5))) | \
                ((yw + f32(0.5)) == np.floor(yw + f32(0.5)))
            if (keep & tie).any():
                seen.add("tie_odd" if size & 1 else "tie_even")
        if (keep & (depth == ro.DEPTH_MAX)).any():
            seen.add("far")
            if (keep & (depth == ro.DEPTH_MAX) & (colour == 255)).any():
                seen.add("empty_key")
            # a far point's sprite over a pixel that a nearer point wins
            keys = ro.scatter_min(keep, x0, y0, depth, colour, W, H, size)
            far = keep & (depth == ro.DEPTH_MAX) & (x0 >= 0) & (x0 < W) & (y0 >= 0) & (y0 < H)
            if (keys[y0[far] * W + x0[far]] >> np.uint32(8) < ro.DEPTH_MAX).any():
                seen.add("far_behind_nearer")
        if (keep & (depth == 0)).any():
            seen.add("near")
        with np.errstate(all="ignore"):
            zw32 = ro.window_fp32(xyz, m, W, H)[2].astype(np.float64)
            v = zw32 * D_MAX
            body = keep & (depth < ro.DEPTH_MAX) & (np.abs(v - np.floor(v) - 0.5) > 0.01)
            if (body & (depth > v)).any():
                seen.add("depth_round_up")
            if (body & (depth < v)).any():
                seen.add("depth_round_down")
        if size > 1:
            if (keep & (x0 < 0) & (x0 + size > 0)).any():
                seen.add("edge_left")
            if (keep & (x0 < W) & (x0 + size > W)).any():
                seen.add("edge_right")
            if (keep & (y0 < 0) & (y0 + size > 0)).any():
                seen.add("edge_bottom")
            if (keep & (y0 < H) & (y0 + size > H)).any():
                seen.add("edge_top")
        k = np.flatnonzero(keep)
        if len(k):
            key = (x0[k] * 1_000_003 + y0[k]) * (1 << 25) + depth[k]
            u, inv, cnt = np.unique(key, return_inverse=True, return_counts=True)
            for g in np.flatnonzero(cnt > 1)[:50]:
                if len(np.unique(colour[k][inv == g])) > 1:
                    seen.add("equal_depth")
                    break
        # a 64-point wavefront whose only visible points lie exactly on a clip plane
        n64 = len(xyz) // 64
        if n64:
            kk = keep[:n64 * 64].reshape(n64, 64)
            on = (keep & (mag == cw))[:n64 * 64].reshape(n64, 64)
            if ((kk.sum(1) > 0) & (kk == on).all(1) & (kk.sum(1) < 64)).any():
                seen.add("box_on_plane")
        fwd.append(np.asarray(m, f32).reshape(4, 4)[2, 3] if keep.any() else 0)   # (column 2, row 3: cw's z coefficient)
        keeps.append(keep)
        ons.append(keep & (mag == cw))
    n64 = len(xyz) // 64
    if len(mvps) > 1 and n64:
        # a wavefront that exactly one view sees, and only through points exactly on that view's plane
        K = np.stack(keeps)[:, :n64 * 64].reshape(len(mvps), n64, 64)
        O = np.stack(ons)[:, :n64 * 64].reshape(len(mvps), n64, 64)
        one_view = (K.any(2).sum(0) == 1)
        only_plane = ((K == O) | ~K).all(2).all(0)
        if (one_view & only_plane).any():
            seen.add("box_at_common_bound")
    if any(f > 0 for f in fwd) and any(f < 0 for f in fwd):
        seen.add("opposed_views")
    return seen


def reached(cases, W, H):
    seen = set()
    for c in cases:
        seen |= branches(c, W, H)
    return seen
