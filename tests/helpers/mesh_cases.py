"""Hard meshes, textures and views for the textured-mesh renderer -- TEST INFRASTRUCTURE ONLY.

families(W, H) -> {name: [case, ...]}; a case is a dict with xyz [3 T, 3] and uv [3 T, 2] float32 (the expanded per-corner arrays),
rgb [h, w, 3] uint8 (the texture), mvps [S, 16] float32 (column-major) and bulk [T] bool: the triangles NOT built on a decision
boundary (the CPU tests require that almost none of their fragments fall inside the twin-vs-model exemption).
branches(case, W, H) -> the branches of the mesh rule the case reaches, computed from the staged fp32 twin
(oracle/mesh_oracle_np.py); EXPECTED_BRANCHES: what each family exists to reach, on frames of at least 64 x 48.

Where a case needs exact window coordinates it uses EXACT, the identity matrix (cx = x, cy = y, cz = z, cw = 1: affine, no
perspective), and corners found by exact_ndc: the fp32 x whose fp32 window coordinate (x / 1 * 0.5 + 0.5) * W IS the wanted
half-integer.  On a power-of-two frame side every step of that is exact in real arithmetic too, so the float64 model sees the same
coordinates; on other sides the model sees them 1e-7 off (and the criterion exempts those fragments, as it must).
Everything else is placed in window coordinates and unprojected through the view's matrix in float64 (rc.unproject).
"""
import functools

import numpy as np

from helpers import render_cases as rc
from oracle import mesh_oracle_np as mo

f32 = np.float32
EXACT = np.eye(4, dtype=f32).reshape(16)
ZN, ZF = rc.ZN, rc.ZF
TEXTURE_SIDES = ((100, 60), (127, 3), (3, 5), (1, 37), (1, 1), (2, 2))   # (w, h)
FAR_FROM_ORIGIN = (0.0, 100.0, 1000.0)


def _step(x, n):
    x = f32(x)
    for _ in range(abs(n)):
        x = np.nextafter(x, f32(np.inf if n > 0 else -np.inf))
    return x


def exact_ndc(t, n):
    """fp32 x with (x * 0.5 + 0.5) * n == t in fp32 arithmetic, or None."""
    x0 = f32(2.0 * t / n - 1.0)
    for k in (0, 1, -1, 2, -2, 3, -3):
        x = _step(x0, k)
        if (x * f32(0.5) + f32(0.5)) * f32(n) == f32(t):
            return x
    return None


def exact_points(W, H, pts, z=0.0):
    """Window points pts [(x, y), ...] shifted by a common whole number of pixels until every one has exact fp32 coordinates under
    EXACT -> (xyz float32 [n, 3], (dx, dy))."""
    for dy in range(0, 6):
        for dx in range(0, 6):
            out = [(exact_ndc(x + dx, W), exact_ndc(y + dy, H)) for x, y in pts]
            if all(a is not None and b is not None for a, b in out):
                return np.array([(a, b, z) for a, b in out], f32), (dx, dy)
    raise AssertionError(f"no exact placement at {W} x {H}")


def solid_texture(n=4):
    """n x n texels whose luma rises along the diagonal: texel (i, i) has its own grey; constant uv at its centre shows it."""
    rgb = np.zeros((n, n, 3), np.uint8)
    for j in range(n):
        for i in range(n):
            rgb[j, i] = 20 + (200 // (n * n)) * (j * n + i)
    return rgb


def texel_uv(i, j, n=4):
    return ((i + 0.5) / n, (j + 0.5) / n)


def noise_texture(w, h, seed=0, lo=0, hi=250):
    rng = np.random.default_rng(seed + 31 * w + h)
    sm = rng.integers(lo, hi + 1, (h, w, 1))
    return np.clip(sm + rng.integers(-5, 6, (h, w, 3)), lo, hi).astype(np.uint8)


def smooth_texture(w, h, seed=0):
    """A texture with gentle slopes (neighbouring texels a few grey levels apart), kept below 250."""
    y, x = np.mgrid[0:h, 0:w]
    g = 120 + 60 * np.sin(2 * np.pi * (x / max(w, 2) + 0.13 * seed)) + 50 * np.cos(2 * np.pi * y / max(h, 2))
    return np.repeat(np.clip(g, 5, 245)[..., None], 3, 2).astype(np.uint8)


def _case(xyz, uv, rgb, mvps, bulk=True, note=""):
    xyz = np.ascontiguousarray(np.asarray(xyz, np.float64).astype(f32).reshape(-1, 3))
    uv = np.ascontiguousarray(np.asarray(uv, np.float64).astype(f32).reshape(-1, 2))
    assert len(xyz) % 3 == 0 and len(uv) == len(xyz), (xyz.shape, uv.shape)
    bulk = np.broadcast_to(np.asarray(bulk, bool), (len(xyz) // 3,)).copy()
    return {"xyz": xyz, "uv": uv, "rgb": np.ascontiguousarray(rgb, np.uint8), "mvps": np.asarray(mvps, f32).reshape(-1, 16).copy(),
            "bulk": bulk, "note": note}


def both_windings(xyz, uv):
    x3, u3 = np.asarray(xyz).reshape(-1, 3, 3), np.asarray(uv).reshape(-1, 3, 2)
    return np.concatenate([x3, x3[:, ::-1]]).reshape(-1, 3), np.concatenate([u3, u3[:, ::-1]]).reshape(-1, 2)


JITTER = (0.137, 0.291)     # keeps corners placed at round fractions of the frame off the pixel centres (a box bound's decision)


def from_window(m, W, H, tris, z=0.5, jitter=JITTER):
    """Triangles given by window corners [(x, y) or (x, y, zw)] * 3 each -> world xyz (float64) under matrix m."""
    pts = np.array([[p[0] + jitter[0], p[1] + jitter[1], p[2] if len(p) > 2 else z] for t in tris for p in t], np.float64)
    return rc.unproject(m, W, H, pts[:, 0], pts[:, 1], pts[:, 2])


def quad(x0, y0, x1, y1):
    """Two counter-clockwise (in y-up window coordinates) triangles."""
    return [[(x0, y0), (x1, y0), (x1, y1)], [(x0, y0), (x1, y1), (x0, y1)]]


def quad_uv(u0, v0, u1, v1):
    return [(u0, v0), (u1, v0), (u1, v1), (u0, v0), (u1, v1), (u0, v1)]


# ------------------------------------------------------------------------------------------------------------ the families
def pixel_centre_figures(W, H):
    """-> list of (name, window triangles with half-integer corners, texel per triangle): shared edges through pixel centres in
    every direction, and a fan about a pixel centre."""
    # (in the upper right quarter of the window: there the fp32 window coordinates are dense enough for most half-integers to be hit)
    s = 12 if min(W, H) >= 64 else 8
    a, b = W // 2 + 0.5, H // 2 + 0.5
    figs = []
    sq = [(a, b), (a + s, b), (a + s, b + s), (a, b + s)]
    figs.append(("diag_up", [[sq[0], sq[1], sq[2]], [sq[0], sq[2], sq[3]]]))          # shared edge at 45 degrees, going up-right
    figs.append(("diag_down", [[sq[0], sq[1], sq[3]], [sq[1], sq[2], sq[3]]]))        # ... going up-left
    h = s // 2
    figs.append(("vertical", quad(a, b, a + h, b + s) + quad(a + h, b, a + s, b + s)))   # two quads side by side
    figs.append(("horizontal", quad(a, b, a + s, b + h) + quad(a, b + h, a + s, b + s)))  # ... one above the other
    c = (a + h, b + h)
    ring = [(c[0] + h * dx, c[1] + h * dy) for dx, dy in ((1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1))]
    figs.append(("fan", [[c, ring[i], ring[(i + 1) % 8]] for i in range(8)]))
    return figs


def _pixel_centres(W, H):
    cases = []
    rgb = solid_texture(4)
    for name, tris in pixel_centre_figures(W, H):
        pts = [p for t in tris for p in t]
        xyz, shift = exact_points(W, H, pts)
        uv = np.array([texel_uv(k % 4, (k // 4 + k) % 4) for k in range(len(tris)) for _ in range(3)])
        c = _case(xyz, uv, rgb, EXACT[None], bulk=False, note=name)
        c["window"] = [[(x + shift[0], y + shift[1]) for x, y in t] for t in tris]
        cases.append(c)
    return cases


def tessellation_mesh(W, H, m, nx=8, ny=6, seed=4, tilt=0.25):
    """A closed, jittered, tilted grid in front of view m: nx x ny quads whose outline (the four unjittered outer corners'
    quadrilateral) lies inside the window, both windings.  -> xyz, uv (float64), outline [4, 3] world corners."""
    rng = np.random.default_rng(seed)
    gx, gy = np.meshgrid(np.linspace(0.08, 0.92, nx + 1), np.linspace(0.1, 0.9, ny + 1))
    inner = np.zeros_like(gx, bool)
    inner[1:-1, 1:-1] = True
    gx = gx + inner * rng.uniform(-0.3, 0.3, gx.shape) / nx
    gy = gy + inner * rng.uniform(-0.3, 0.3, gy.shape) / ny
    # the corners lie in one world plane: unproject three of the outline's corners, the rest by the plane's parameters
    o = rc.unproject(m, W, H, 0.08 * W, 0.1 * H, 0.55)
    ex = rc.unproject(m, W, H, 0.92 * W, 0.1 * H, 0.55 + tilt) - o
    ey = rc.unproject(m, W, H, 0.08 * W, 0.9 * H, 0.55 + 0.4 * tilt) - o
    s, t = (gx - 0.08) / 0.84, (gy - 0.1) / 0.8
    P = o + s[..., None] * ex + t[..., None] * ey
    tris, uvs = [], []
    for j in range(ny):
        for i in range(nx):
            p = [P[j, i], P[j, i + 1], P[j + 1, i + 1], P[j + 1, i]]
            q = [(1.7 * s[j, i], 1.3 * t[j, i]), (1.7 * s[j, i + 1], 1.3 * t[j, i + 1]), (1.7 * s[j + 1, i + 1], 1.3 * t[j + 1, i + 1]),
                 (1.7 * s[j + 1, i], 1.3 * t[j + 1, i])]
            tris += [p[0], p[1], p[2], p[0], p[2], p[3]]
            uvs += [q[0], q[1], q[2], q[0], q[2], q[3]]
    xyz, uv = both_windings(np.array(tris), np.array(uvs))
    return xyz, uv, np.array([P[0, 0], P[0, -1], P[-1, -1], P[-1, 0]])


def tessellation_views(W, H):
    cams = rc.cameras(W, H)
    return np.stack([cams["axis"], rc.shifted(cams["axis"][None], (0.4, -0.3, 1.0))[0], cams["rolled"],
                     rc.shifted(cams["oblique"][None], (-0.5, 0.2, 2.0))[0]])


def _tessellation(W, H):
    views = tessellation_views(W, H)
    xyz, uv, outline = tessellation_mesh(W, H, views[0])
    c = _case(xyz, uv, smooth_texture(100, 60), views, note="closed jittered grid")
    c["outline"] = outline
    return [c]


def _degenerate(W, H):
    m = rc.cameras(W, H)["axis"]
    w, h = float(W), float(H)
    back = quad(0.1 * w, 0.1 * h, 0.9 * w, 0.9 * h)
    bad = [
        [(10.2, 10.3), (10.2, 10.3), (10.2, 10.3)],                                    # one point three times
        [(12.2, 8.3), (30.7, 20.1), (30.7, 20.1)],                                     # a repeated corner
        [(5.0, 5.0), (15.0, 10.0), (25.0, 15.0)],                                      # collinear
        [(0.2 * w, 20.6), (0.8 * w, 20.6), (0.8 * w, 21.4)],                           # slivers between two rows / columns of pixel centres
        [(0.2 * w, 20.6), (0.8 * w, 21.4), (0.2 * w, 21.4)],
        [(30.6, 0.2 * h), (31.4, 0.2 * h), (31.4, 0.8 * h)],
        [(3.3, 4.2), (3.3 + 0.9 * w, 4.2 + 0.7 * h), (3.3 + 0.9 * w - 4e-4, 4.2 + 0.7 * h + 5e-4)],   # needles: under 1e-3 px wide
        [(7.7, 0.9 * h), (7.7 + 0.8 * w, 0.9 * h - 0.6 * h), (7.7 + 0.8 * w + 3e-4, 0.9 * h - 0.6 * h + 4e-4)],
    ]
    xyz = from_window(m, W, H, bad, z=0.4)
    uvb = np.resize(np.array([(0.1, 0.2), (0.9, 0.3), (0.4, 0.8)]), (len(bad) * 3, 2))
    xyz, uvb = both_windings(xyz, uvb)
    # fp32 area a few ulps from 0 on either side: collinear corners under EXACT, the middle one walked over adjacent floats
    a, b = exact_ndc(8.5, W) or f32(17.0 / W - 1), exact_ndc(40.5, W) or f32(81.0 / W - 1)
    near0 = []
    for k in (-3, -1, 0, 1, 3):
        near0 += [(a, f32(-0.5), 0.1), (b, f32(0.25), 0.1), (f32((float(a) + float(b)) / 2), _step(f32(-0.125), k), 0.1)]
    xb = from_window(m, W, H, back, z=0.7)
    ub = np.array(quad_uv(0, 0, 1.5, 1.2))
    cases = [_case(np.concatenate([xb, xyz]), np.concatenate([ub, uvb]), smooth_texture(100, 60, 1), m[None],
                   bulk=np.r_[np.ones(2, bool), np.zeros(len(xyz) // 3, bool)], note="zero area, slivers, needles over a quad")]
    n0 = np.array(near0, f32)
    n0, u0 = both_windings(n0, np.resize(np.array([(0.1, 0.2), (0.9, 0.3), (0.4, 0.8)]), (len(n0), 2)))
    cases.append(_case(n0, u0, smooth_texture(100, 60, 1), EXACT[None], bulk=False, note="area within ulps of 0"))
    return cases


SMALL_BOXES = ((4, 4), (1, 16), (16, 1), (2, 8), (17, 1), (1, 17), (3, 5), (5, 3))   # (w, h): 16, 16, 16, 16, 17, 17, 15, 15 pixels


def _small_box(W, H):
    m = rc.cameras(W, H)["axis"]
    tris, spots = [], [(6, 5)]
    for sx, sy in ((62, 5), (5, 62), (62, 62), (W - 1, 9), (9, H - 1), (W - 1, H - 1), (W - 4, H - 3)):
        spots.append((sx, sy))           # across the tile borders x = 63|64, y = 63|64; the last partial tile and dword
    for bw, bh in SMALL_BOXES:
        for k, (sx, sy) in enumerate(spots):
            x0, y0 = min(sx, W - bw), min(sy, H - bh)           # first pixel of the box (kept inside the window)
            x0, y0 = max(0, x0 - (bw // 2 if k in (1, 3) else 0)), max(0, y0 - (bh // 2 if k in (2, 3) else 0))   # straddle the border
            xa, xb, ya, yb = x0 + 0.3, x0 + bw - 1 + 0.62, y0 + 0.27, y0 + bh - 1 + 0.71     # (the diagonal misses the pixel centres)
            tris.append([(xa, ya), (xb, ya), (xb, yb)])
            tris.append([(xa, ya), (xb, yb), (xa, yb)])
    zs = np.repeat(np.linspace(0.2, 0.8, len(tris)), 3)
    pts = np.array([p for t in tris for p in t])
    xyz = rc.unproject(m, W, H, pts[:, 0], pts[:, 1], zs)      # (no jitter: the boxes are placed to the pixel)
    uv = np.resize(np.array([(0.05, 0.1), (0.3, 0.12), (0.28, 0.4)]), (len(xyz), 2)) + np.repeat(np.arange(len(tris)) * 0.137, 3)[:, None]
    return [_case(xyz, uv, smooth_texture(100, 60, 2), m[None], note="boxes of 15, 16, 17 pixels")]


FULL_BINS = (127, 128, 255, 256, 300)


def _full_bins(W, H):
    m = rc.cameras(W, H)["axis"]
    cases = []
    e = float(min(W, H, 64) - 6)
    for n in FULL_BINS:
        for equal in (False, True):
            rng = np.random.default_rng(n + equal)
            tris, zs = [], []
            for k in range(n):
                ox, oy = rng.uniform(2.1, 3.9, 2)
                tris.append([(ox, oy), (ox + e, oy), (ox + (e if k & 1 else 0), oy + e)])
                zs += [0.5 if equal else 0.2 + 0.6 * ((k * 37) % n) / n] * 3
            pts = np.array([p for t in tris for p in t])
            xyz = rc.unproject(m, W, H, pts[:, 0], pts[:, 1], np.array(zs))
            uv = np.repeat(np.array([texel_uv(k % 4, (k // 4) % 4) for k in range(n)]), 3, 0)
            cases.append(_case(xyz, uv, solid_texture(4), m[None], note=f"{n} triangles over one tile, {'equal' if equal else 'distinct'} depths"))
            # the bin counts matter to the kernels; the float64 criterion needs one distinct-depth and one equal-depth case
            cases[-1]["criterion"] = n == 128
    return cases


def near_plane_corner(m, W, H, xw, yw):
    """World points on the near plane of view m at window (xw, yw): fp32 d = cz + cw exactly 0 if such a float exists, and its
    one-step neighbours along z -> (on or None, below, above)."""
    P = rc.unproject(m, W, H, xw, yw, 0.0).astype(f32)

    def d(p):
        c = mo.clip_coords(np.repeat(p[None], 3, 0), m)
        return float(f32(c[2][0, 0]) + f32(c[3][0, 0]))

    best = None
    for k in range(-40, 41):
        q = P.copy()
        q[2] = _step(P[2], k)
        if d(q) == 0.0:
            best = q
            break
    ref = best if best is not None else P
    lo, hi = ref.copy(), ref.copy()
    lo[2], hi[2] = _step(ref[2], -1), _step(ref[2], 1)
    return best, lo, hi


def _near_plane(W, H):
    from test_render import ground_mesh
    cams = rc.cameras(W, H)
    m = cams["axis"]
    w, h = float(W), float(H)
    tex = smooth_texture(100, 60, 3)

    def world(x, y, z):    # window x, y at eye depth z (may be in front of the near plane or behind the eye)
        p = rc.unproject(m, W, H, x + JITTER[0], y + JITTER[1], 0.5)
        return p * (z / p[2])

    tris, uvs, bulk = [], [], []

    def add(p, q, b=True):
        tris.extend(p)
        uvs.extend(q)
        bulk.append(b)
    t3 = [(0.1, 0.1), (0.9, 0.2), (0.3, 0.95)]
    add([world(0.2 * w, 0.2 * h, 12), world(0.4 * w, 0.25 * h, 12), world(0.3 * w, 0.6 * h, 3.0)], t3)     # 2 corners inside
    add([world(0.5 * w, 0.2 * h, 12), world(0.6 * w, 0.5 * h, 2.0), world(0.45 * w, 0.5 * h, 2.5)], t3)    # 1 corner inside
    # two triangles sharing the edge that crosses the plane: both cut it at the same point
    a, b = world(0.7 * w, 0.3 * h, 9.0), world(0.8 * w, 0.7 * h, 3.0)
    add([a, b, world(0.6 * w, 0.7 * h, 6.0)], t3)
    add([b, a, world(0.95 * w, 0.5 * h, 6.0)], t3)
    # small after clipping: a tip that reaches a few pixels inside the near plane
    add([world(0.2 * w, 0.8 * h, ZN * 1.4), world(0.2 * w + 40, 0.8 * h + 6, 2.0), world(0.2 * w + 40, 0.8 * h - 6, 2.0)], t3)
    # crosses the near and the far plane; through the eye (a corner behind the camera: cw < 0)
    add([world(0.5 * w, 0.7 * h, 2.0), world(0.7 * w, 0.8 * h, 60.0), world(0.4 * w, 0.95 * h, 60.0)], t3)
    add([world(0.1 * w, 0.5 * h, 20.0), world(0.3 * w, 0.5 * h, 20.0), np.array([0.5, 1.0, -4.0])], t3)
    xyz, uv = both_windings(np.array(tris), np.array(uvs))
    cases = [_case(xyz, uv, tex, np.stack([m, rc.shifted(m[None], (0.1, -0.05, 0.4))[0]]), bulk=bulk + bulk, note="crossing triangles")]
    # corners with d == 0 and one fp32 step either side
    t2, u2 = [], []
    for i, x in enumerate((0.2, 0.5, 0.8)):
        on, lo, hi = near_plane_corner(m, W, H, x * w, 0.5 * h)
        for p in (on, lo, hi):
            if p is not None:
                t2 += [world(x * w - 8, 0.3 * h, 9.0), world(x * w + 8, 0.3 * h, 9.0), p.astype(np.float64)]
                u2 += t3
    x2, u2 = both_windings(np.array(t2), np.array(u2))
    cases.append(_case(x2, u2, tex, m[None], bulk=False, note="a corner on the near plane and a step either side"))
    gx, gu, grgb, _ = ground_mesh(W, H)
    gx, gu = both_windings(gx, gu)
    cases.append(_case(gx, gu, grgb, np.stack([m, rc.shifted(m[None], (0.4, -0.3, 1.0))[0]]), note="ground under the camera, a wall beside it"))
    return cases


PLANES = ("left", "right", "bottom", "top", "near", "far")     # block_frustum_cull's bit order: cx < -cw, cx > cw, cy < -cw, cy > cw, cz < -cw, cz > cw


def cull_code(block_xyz, m):
    """block_frustum_cull of nmi_mesh.hip for one block of triangles, restated in fp32 -> bit p set: every corner of the block's box
    is beyond plane p by more than the 1e-5 margin (the block skips the view)."""
    P = np.asarray(block_xyz, f32).reshape(-1, 3)
    m = np.asarray(m, f32)
    lo, hi = P.min(0), P.max(0)
    a = np.maximum(np.abs(lo), np.abs(hi))
    mw = np.abs(m[3]) * a[0] + np.abs(m[7]) * a[1] + np.abs(m[11]) * a[2] + np.abs(m[15])
    e = [f32(1e-5) * (np.abs(m[r]) * a[0] + np.abs(m[4 + r]) * a[1] + np.abs(m[8 + r]) * a[2] + np.abs(m[12 + r]) + mw) for r in range(3)]
    code = 0x3F
    for c in range(8):
        b = [hi[k] if (c >> k) & 1 else lo[k] for k in range(3)]
        cl = [(m[r] * b[0] + m[4 + r] * b[1]) + (m[8 + r] * b[2] + m[12 + r]) for r in range(4)]
        cc = 0
        for r in range(3):
            cc |= (1 << (2 * r)) if cl[r] + cl[3] < -e[r] else 0
            cc |= (2 << (2 * r)) if cl[3] - cl[r] < -e[r] else 0
        code &= cc
    return code


def block_256(m, W, H, x0, x1, y0, y1, zw=0.5):
    """16 x 8 quads = 256 triangles (one block of the binning pass) over the window rectangle, at one window depth."""
    xs, ys = np.linspace(x0, x1, 17), np.linspace(y0, y1, 9)
    tris = [t for j in range(8) for i in range(16) for t in quad(xs[i], ys[j], xs[i + 1], ys[j + 1])]
    uv = np.array([q for j in range(8) for i in range(16) for q in quad_uv(i / 16, j / 8, (i + 1) / 16, (j + 1) / 8)])
    return from_window(m, W, H, tris, z=zw, jitter=(0.0, 0.0)), uv


def _frustum_margin(W, H):
    """Blocks of 256 triangles (the block cull's unit) at each of the six clip planes.  Side planes: one block whose box ends inside
    the last pixel column / row (visible: must be drawn) and one just beyond the plane, within the cull's 1e-5 margin (the cull
    keeps it, every triangle is dropped by its own test).  Near and far: a block ON the plane (drawn, at depth 0 / 2^24 - 1) and one
    just beyond it within the margin.  Counts of 1, 255, 256 and 257 triangles; 64, 65 and 130 views."""
    from test_render import plane_mesh
    m = rc.cameras(W, H)["axis"]
    w, h = float(W), float(H)
    tex = smooth_texture(100, 60, 8)
    cases = []
    for depth in (ZF, ZN):
        x, u, rgb, _ = plane_mesh(W, H, depth=depth, nx=16, ny=8)
        for n in (1, 255, 256, 257):
            cases.append(_case(x[:3 * n], u[:3 * n], np.minimum(rgb, 250), m[None], bulk=False, note=f"{n} triangles at z = {depth}"))
            cases[-1]["criterion"] = n == 256        # (the counts around a block are the kernels' business)
    # beyond the far / near plane by 2e-5 / 1e-5 of the depth: cz - cw (cz + cw) is a few fp32 steps beyond 0 and a fraction of the margin
    for depth, name in ((ZF * (1 + 2e-5), "far"), (ZN * (1 - 1e-5), "near")):
        x, u, rgb, _ = plane_mesh(W, H, depth=depth, nx=16, ny=8)
        cases.append(_case(x[:3 * 256], u[:3 * 256], np.minimum(rgb, 250), m[None], bulk=False, note=f"block just beyond the {name} plane"))
    lo, hi = 1e-6, 5e-6        # of the frame's side: 2e-6 .. 1e-5 in clip units, inside the margin of ~2e-5 cw, many fp32 steps wide
    for name, vis, out in (("left", (0.2, 5.3, 0.2 * h, 0.8 * h), (-hi * w, -lo * w, 0.2 * h, 0.8 * h)),
                           ("right", (w - 5.3, w - 0.2, 0.2 * h, 0.8 * h), (w + lo * w, w + hi * w, 0.2 * h, 0.8 * h)),
                           ("bottom", (0.2 * w, 0.8 * w, 0.2, 5.3), (0.2 * w, 0.8 * w, -hi * h, -lo * h)),
                           ("top", (0.2 * w, 0.8 * w, h - 5.3, h - 0.2), (0.2 * w, 0.8 * w, h + lo * h, h + hi * h))):
        x, u = block_256(m, W, H, *vis)
        cases.append(_case(x, u, tex, m[None], note=f"block ending inside the last pixels at the {name} plane"))
        x, u = block_256(m, W, H, *out)
        cases.append(_case(x, u, tex, m[None], bulk=False, note=f"block just beyond the {name} plane"))
    x, u, rgb, _ = plane_mesh(W, H, depth=11.0, nx=3, ny=2)
    for S in (64, 65, 130):
        views = np.concatenate([rc.shifted(m[None], (0.3 * np.sin(s), 0.2 * np.cos(2.0 * s), 0.02 * s)) for s in range(S)])
        cases.append(_case(x, u, np.minimum(rgb, 250), views, note=f"{S} views"))
        cases[-1]["criterion"] = S == 130
    return cases


def _depth(W, H):
    from test_render import plane_mesh
    from test_render_edges import _far_and_near_mesh
    m = rc.cameras(W, H)["axis"]
    w, h = float(W), float(H)
    # two planes through each other: a line of near ties
    a = from_window(m, W, H, [[(0.1 * w, 0.1 * h, 0.3), (0.9 * w, 0.1 * h, 0.7), (0.9 * w, 0.9 * h, 0.7)],
                              [(0.1 * w, 0.1 * h, 0.3), (0.9 * w, 0.9 * h, 0.7), (0.1 * w, 0.9 * h, 0.3)],
                              [(0.1 * w, 0.1 * h, 0.7), (0.9 * w, 0.1 * h, 0.3), (0.9 * w, 0.9 * h, 0.3)],
                              [(0.1 * w, 0.1 * h, 0.7), (0.9 * w, 0.9 * h, 0.3), (0.1 * w, 0.9 * h, 0.7)]])
    ua = np.array(quad_uv(0, 0, 1, 1) + quad_uv(0.4, 0.3, 1.9, 1.6))
    cases = [_case(a, ua, smooth_texture(100, 60, 5), np.stack([m, rc.shifted(m[None], (0.2, 0.1, 0.5))[0]]), note="interpenetrating planes")]
    # coplanar copies (test_render._coplanar_scene's idea, fewer triangles): every pixel an exact tie; draw order decides
    xa, ua_, rgb, _ = plane_mesh(W, H, nx=3, ny=2)
    xb, ub, _, _ = plane_mesh(W, H, nx=9, ny=7)
    xa, ua_, xb, ub = xa[:36], ua_[:36], xb[:3 * 2 * 63], (ub[:3 * 2 * 63] + f32(0.37)).astype(f32)
    for first, second in (((xa, ua_), (xb, ub)), ((xb, ub), (xa, ua_))):
        cases.append(_case(np.concatenate([first[0], second[0]]), np.concatenate([first[1], second[1]]), np.minimum(rgb, 250), m[None],
                           bulk=False, note="coplanar copies"))
    xf, uf, xn, un, rgb, _ = _far_and_near_mesh(W, H)
    cases.append(_case(np.concatenate([xf, xn]), np.concatenate([uf, un]), np.minimum(rgb, 250), m[None],
                       bulk=np.r_[np.zeros(len(xf) // 3, bool), np.ones(len(xn) // 3, bool)], note="far plane behind a nearer plane"))
    # a tilted quad next to the near plane under EXACT (cw = 1: zw = z / 2 + 1/2 without a rounding that matters): z (2^24 - 1) is a
    # few tens of thousands, its fp32 roundings a hundredth of a step, so round-to-nearest and truncation can be told apart
    q = from_window(EXACT, W, H, [[(0.1 * w, 0.1 * h, 0.002), (0.9 * w, 0.12 * h, 0.005), (0.88 * w, 0.9 * h, 0.008)],
                                  [(0.1 * w, 0.1 * h, 0.002), (0.88 * w, 0.9 * h, 0.008), (0.12 * w, 0.88 * h, 0.004)]])
    cases.append(_case(q, np.array(quad_uv(0, 0, 1, 1)), smooth_texture(100, 60, 5), EXACT[None], note="depth rounding next to the near plane"))
    return cases


def _texture(W, H):
    m = rc.cameras(W, H)["axis"]
    w, h = float(W), float(H)
    cases = []
    n = min(32, min(W, H) - 8)
    for tw_, th_ in TEXTURE_SIDES:
        rgb = noise_texture(tw_, th_, 1)
        rgb[0, 0] = 0            # a luma-0 and a luma-1 texel: grey 255 on a covered pixel
        rgb[-1, -1] = 255
        # whole-pixel corners: with one texel per pixel the pixel centres sample texel centres (u w - 0.5 a whole number: the floor's
        # decision), or texel borders when the uv origin is half a texel off
        xyz = from_window(EXACT, W, H, quad(4.0, 4.0, 4.0 + n, 3.0 + n), jitter=(0.0, 0.0))   # (n x (n - 1): the diagonal misses the pixel centres)
        # (a) one texel per pixel on the longer side: rho2 about 1, sample points on texel centres -- and on texel borders when the
        # uv origin is half a texel off; (b) integer uv at the corners, minified by the texture's size; (c) x 50 magnification
        k, k1 = float(n), float(n - 1)
        uv_sets = [quad_uv(0.0, 0.0, k / tw_, k1 / th_), quad_uv(0.5 / tw_, 0.5 / th_, (k + 0.5) / tw_, (k1 + 0.5) / th_),
                   quad_uv(-2.0, -1.0, 3.0, 2.0), quad_uv(0.25, 0.25, 0.25 + k / (50.0 * tw_), 0.25 + k1 / (50.0 * th_)),
                   quad_uv(500.0, -500.0, 500.0 + 2 * k / tw_, -500.0 + 2 * k1 / th_), quad_uv(0.0, 0.0, 300.0, 300.0)]
        for uvq in uv_sets:
            cases.append(_case(xyz, np.array(uvq), rgb, EXACT[None], note=f"{tw_}x{th_} quad"))
    # a grazing plane: strong, anisotropic minification towards the horizon, seen in perspective
    g = from_window(m, W, H, [[(0.05 * w, 0.05 * h, 0.05), (0.95 * w, 0.05 * h, 0.05), (0.8 * w, 0.6 * h, 0.995)],
                              [(0.05 * w, 0.05 * h, 0.05), (0.8 * w, 0.6 * h, 0.995), (0.2 * w, 0.6 * h, 0.995)]])
    cases.append(_case(g, np.array(quad_uv(0, 0, 6, 40)), noise_texture(100, 60, 2), m[None], note="grazing plane"))
    cases.append(_case(g, np.array(quad_uv(0, 0, 6, 40)), noise_texture(127, 3, 2), m[None], note="grazing plane, 127x3"))
    return cases


RCP_EXPONENTS = (120, 121, -129, -130)


def _reciprocal_range(W, H):
    """warp_rcp_ok takes floats whose exponent field is in [3, 252]: 2^-124 <= |Q| < 2^126.  The view's matrix times 2^k scales
    cw = z_eye 2^k and Q = 1 / cw by powers of two and nothing else.  With z_eye in [8, 16): k = 120 gives Q in (2^-124, 2^-123]
    (inside), k = 121 Q in (2^-125, 2^-124] (outside: the division), k = -129 Q in (2^125, 2^126] (inside but for Q = 2^126),
    k = -130 Q in (2^126, 2^127] (outside; cw is subnormal there)."""
    m = rc.cameras(W, H)["axis"]
    w, h = float(W), float(H)
    tris = quad(0.15 * w, 0.15 * h, 0.85 * w, 0.85 * h)
    world = from_window(m, W, H, tris, z=0.5)
    world = world * (11.0 / world[:, 2:3])      # z_eye = 11
    uv = np.array(quad_uv(0.1, 0.2, 2.3, 1.7))
    rgb = smooth_texture(100, 60, 6)
    cases = [_case(world, uv, rgb, (m.astype(np.float64) * 2.0 ** k).astype(f32)[None], bulk=(k > -130), note=f"matrix x 2^{k}")
             for k in RCP_EXPONENTS]
    # a wall along the view direction under a camera with a very far far plane: its vanishing line is a column of the image, and
    # next to it the right-hand neighbour sample lies beyond it (Q + qx <= 0 < Q)
    far = rc.mvp(W, H, (0, 0, 0), (0, 0, 1), (0, -1, 0), zn=0.5, zf=4e6)
    wall = np.array([(-1.0, -3.0, 1.0), (-1.0, 3.0, 1.0), (-1.0, 3.0, 3e6), (-1.0, -3.0, 1.0), (-1.0, 3.0, 3e6), (-1.0, -3.0, 3e6)])
    wx, wu = both_windings(wall, np.array([(0, 0), (0, 1), (50, 1), (0, 0), (50, 1), (50, 0)], np.float64))
    for mirror in (1.0, -1.0):
        cases.append(_case(wx * [mirror, 1, 1], wu, noise_texture(127, 3, 3), far[None], bulk=False, note="wall towards its vanishing line"))
    return cases


def _nonfinite(W, H):
    m = rc.cameras(W, H)["axis"]
    w, h = float(W), float(H)
    good = from_window(m, W, H, quad(0.1 * w, 0.1 * h, 0.6 * w, 0.7 * h) + quad(0.5 * w, 0.4 * h, 0.9 * w, 0.9 * h), z=0.5)
    gu = np.array(quad_uv(0, 0, 1, 1) + quad_uv(0.2, 0.1, 1.4, 0.8))
    base = from_window(m, W, H, [[(0.3 * w, 0.3 * h), (0.7 * w, 0.35 * h), (0.5 * w, 0.8 * h)]], z=0.3)
    bad_x, bad_u = [], []
    t3 = np.array([(0.1, 0.1), (0.9, 0.2), (0.3, 0.95)])
    for corner, comp, val in ((0, 0, np.nan), (1, 1, np.inf), (2, 2, -np.inf), (0, 2, np.nan), (1, 0, np.inf), (2, 2, np.inf)):
        p = base.copy()
        p[corner, comp] = val
        bad_x.append(p)
        bad_u.append(t3)
    bx, bu = both_windings(np.concatenate(bad_x), np.concatenate(bad_u))
    # finite corners, non-finite uv: the triangle is drawn (it covers its pixels and hides what is behind) with grey 0
    uvbad = []
    for val in (np.nan, np.inf, -np.inf):
        q = t3.copy()
        q[1, 0] = val
        uvbad.append(q)
    front = np.concatenate([from_window(m, W, H, [[(0.15 * w + 20 * i, 0.2 * h), (0.15 * w + 20 * i + 15, 0.2 * h), (0.15 * w + 20 * i, 0.2 * h + 15)]],
                                        z=0.2) for i in range(3)])
    fx, fu = both_windings(front, np.concatenate(uvbad))
    xyz = np.concatenate([good, bx, fx])
    uv = np.concatenate([gu, bu, fu])
    bulk = np.r_[np.ones(4, bool), np.zeros(len(bx) // 3 + len(fx) // 3, bool)]
    return [_case(xyz, uv, smooth_texture(100, 60, 7), np.stack([m, rc.cameras(W, H)["oblique"]]), bulk=bulk, note="NaN / inf corners and uv")]


HUGE_UV = (2.0e7, 1.0e9, 3.0e9, 1.0e11, 1.0e19, 1.0e30, 3.0e38)


def _huge_uv(W, H):
    """Finite uv beyond the wrap's domain (|u w - 0.5| >= 2^24 - w) on textures whose sides -- and whose small levels' sides -- are
    not powers of two.  Only ever rendered by a library whose wrap_index is bounded."""
    m = rc.cameras(W, H)["axis"]
    w, h = float(W), float(H)
    cases = []
    for tw_, th_ in ((100, 60), (3, 5), (127, 3), (1, 37)):
        tris, uvs = [], []
        for i, big in enumerate(HUGE_UV):
            x0 = 0.05 * w + (0.9 * w / len(HUGE_UV)) * i
            s = 1.0 if i & 1 else -1.0
            tris += quad(x0, 0.1 * h, x0 + 0.1 * w, 0.5 * h)          # uv that changes across the quad: minified to the top level
            uvs += quad_uv(s * big, -s * big, s * big * 1.0001 + 3.0, -s * big * 0.9999 + 2.0)
            tris += quad(x0, 0.5 * h, x0 + 0.1 * w, 0.9 * h)          # one uv at all corners: no footprint, the base level
            uvs += quad_uv(s * big, -s * big, s * big, -s * big)
        cases.append(_case(from_window(m, W, H, tris, z=0.5), np.array(uvs), noise_texture(tw_, th_, 4), m[None], bulk=False,
                           note=f"huge uv on {tw_}x{th_}"))
    return cases


def _far_from_origin(W, H):
    views = tessellation_views(W, H)
    xyz, uv, outline = tessellation_mesh(W, H, views[0])
    cases = []
    for dist in FAR_FROM_ORIGIN:
        t = np.array([0.6, -0.3, 0.74]) / np.linalg.norm([0.6, -0.3, 0.74]) * dist
        c = _case(xyz + t, uv, smooth_texture(100, 60), rc.shifted(views, -t), note=f"{dist:g} m from the origin")
        c["distance"] = dist
        cases.append(c)
    return cases


BUILDERS = {
    "pixel_centres": _pixel_centres, "tessellation": _tessellation, "degenerate": _degenerate, "small_box": _small_box,
    "full_bins": _full_bins, "near_plane": _near_plane, "frustum_margin": _frustum_margin, "depth": _depth, "texture": _texture,
    "reciprocal_range": _reciprocal_range, "nonfinite": _nonfinite, "huge_uv": _huge_uv, "far_from_origin": _far_from_origin,
}


@functools.lru_cache(maxsize=None)
def family(name, W, H):
    return BUILDERS[name](W, H)


def families(W, H):
    return {name: family(name, W, H) for name in BUILDERS}


EXPECTED_BRANCHES = {
    "pixel_centres": {"owned_zero", "unowned_zero", "negative_zero", "shared_edge_one_owner"},
    "tessellation": {"shared_edges", "both_windings"},
    "degenerate": {"area_zero", "area_negative", "area_tiny_positive", "kept_without_fragment", "needle"},
    "small_box": {"box_15", "box_16", "box_17"},
    "full_bins": {"bin_127", "bin_128", "bin_255", "bin_256", "bin_300", "equal_depths"},
    "near_plane": {"one_inside", "two_inside", "d_zero", "d_one_step", "corner_behind_eye", "z_above_one", "small_piece"},
    "frustum_margin": {"block_on_far_plane", "block_on_near_plane", "views_65", "views_130", "ntri_257"}
    | {f"outside_within_margin_{p}" for p in PLANES} | {f"visible_at_{p}" for p in PLANES[:4]},
    "depth": {"equal_depths", "far_depth", "near_tie"},
    "texture": {"odd_sides", "magnified", "minified", "top_level", "wrap_path", "negative_uv", "rho2_one", "rho2_above_one",
                "rho2_below_one", "integer_lambda", "texel_border", "texel_border_step", "grey_255_covered", "grey_0"},
    "reciprocal_range": {"rcp_division", "rcp_fast", "neighbour_beyond_horizon"},
    "nonfinite": {"nan_corner", "inf_corner", "nan_luma"},
    "huge_uv": {"beyond_wrap_domain", "odd_level"},
    "far_from_origin": {"shared_edges"},
}


def _exp_field(x):
    return (np.asarray(x, f32).view(np.uint32) >> np.uint32(23)) & np.uint32(0xFF)


def branches(case, W, H, staged=None):
    """The branches the case reaches, from the staged fp32 twin (one staged render per view)."""
    seen = set()
    levels = mo.mip_luma(case["rgb"])
    S = len(case["mvps"])
    ntri = len(case["xyz"]) // 3
    if S >= 65:
        seen.add("views_65")
    if S >= 130:
        seen.add("views_130")
    if ntri == 257:
        seen.add("ntri_257")
    if any(s & (s - 1) for l in levels for s in l.shape):
        seen.add("odd_sides")
    with np.errstate(all="ignore"):
        if np.isnan(case["xyz"]).any():
            seen.add("nan_corner")
        if np.isinf(case["xyz"]).any():
            seen.add("inf_corner")
        if (case["uv"] < 0).any():
            seen.add("negative_uv")
    views = range(S) if S < 8 else (0, S - 1)
    for s in views:
        st = staged[s] if staged is not None else mo.render_staged(case["xyz"], case["uv"], levels, case["mvps"][s], W, H, keep_cover=True)
        cov = st["covered"]
        kept = [p for p in st["pieces"] if p["t"]["status"] == "kept"]
        status = [p["t"]["status"] for p in st["pieces"]]
        with np.errstate(all="ignore"):
            cw = mo.clip_coords(case["xyz"], case["mvps"][s])[3]
            if any((cw[p["tri"]] <= 0).any() for p in kept):
                seen.add("corner_behind_eye")     # (clipped away with the rest of what is in front of the near plane)
        for p in st["pieces"]:
            t = p["t"]
            if p["n_in"] == 1:
                seen.add("one_inside")
            if p["n_in"] == 2:
                seen.add("two_inside")
            d = p["d"]
            with np.errstate(all="ignore"):
                if (d == 0).any() and p["n_in"] > 0:
                    seen.add("d_zero")
                if ((d != 0) & (np.abs(d) <= np.spacing(np.abs(p["clip"][3]).max()))).any() and p["n_in"] > 0:
                    seen.add("d_one_step")
            if t["status"] in ("kept", "box") and 0 < float(t["area"]) < 1e-3:
                seen.add("area_tiny_positive")
            if t["status"] == "area":
                seen.add("area_zero" if t["area"] == 0 else "area_negative")
            if t["status"] != "kept":
                continue
            c = p["cover"]
            box = (t["x_hi"] - t["x_lo"] + 1) * (t["y_hi"] - t["y_lo"] + 1)
            if box in (15, 16, 17):
                seen.add(f"box_{box}")
            if p["n_in"] < 3 and box <= 16:
                seen.add("small_piece")
            if not c["inside"].any():
                seen.add("kept_without_fragment")
            if float(t["inv_area"]) > 1.0 and max(t["x_hi"] - t["x_lo"], t["y_hi"] - t["y_lo"]) > 0.5 * min(W, H):
                seen.add("needle")
            zero = [(c["b"][k] == 0) for k in range(3)]
            for k in range(3):
                others = np.ones(zero[k].shape, bool)
                for j in range(3):
                    if j != k:
                        others &= c["b"][j] >= 0
                if (zero[k] & others).any():
                    seen.add("owned_zero" if t["own"][k] else "unowned_zero")
                    if (zero[k] & np.signbit(c["b"][k])).any():
                        seen.add("negative_zero")
            with np.errstate(all="ignore"):
                edge_ok = np.ones(c["z"].shape, bool)
                for k in range(3):
                    edge_ok &= (c["b"][k] > 0) | ((c["b"][k] == 0) & t["own"][k])
                if (edge_ok & (c["z"] > 1)).any():
                    seen.add("z_above_one")
            if (c["inside"] & (c["depth"] == mo.DEPTH_MAX)).any():
                seen.add("far_depth")
            if (c["inside"] & (c["depth"] == 0)).any():
                seen.add("near_depth")
        nf = st["nfrag"]
        if len(kept) > 1 and (nf > 0).any() and (nf[nf > 0] == 1).all():
            seen.add("shared_edge_one_owner")
        if len(kept) > 20 and (nf > 0).any():
            seen.add("shared_edges")
        if "area" in status and "kept" in status:
            seen.add("both_windings")
        # bins: triangles with a large box over the first tile
        big = sum(1 for p in kept if (p["t"]["x_hi"] - p["t"]["x_lo"] + 1) * (p["t"]["y_hi"] - p["t"]["y_lo"] + 1) > 16 and p["t"]["x_lo"] < 64
                  and p["t"]["y_lo"] < 64)
        if big in (127, 128, 255, 256, 300):
            seen.add(f"bin_{big}")
        # equal depths between different triangles on one pixel, and near ties
        if kept:
            d1 = np.full((H, W), -1, np.int64)
            for p in kept:
                t, c = p["t"], p["cover"]
                sub = d1[t["y_lo"]:t["y_hi"] + 1, t["x_lo"]:t["x_hi"] + 1]
                if (c["inside"] & (sub == c["depth"])).any():
                    seen.add("equal_depths")
                if (c["inside"] & (sub >= 0) & (np.abs(sub - c["depth"]) <= 2) & (sub != c["depth"])).any():
                    seen.add("near_tie")
                sub[c["inside"]] = c["depth"][c["inside"]]
        if ntri == 256:
            code = cull_code(case["xyz"], case["mvps"][s])
            cc = mo.clip_coords(case["xyz"], case["mvps"][s])
            beyond = [cc[0] < -cc[3], cc[0] > cc[3], cc[1] < -cc[3], cc[1] > cc[3], cc[2] < -cc[3], cc[2] > cc[3]]
            edge = [cov[:, 0], cov[:, -1], cov[0], cov[-1]]
            for k, name in enumerate(PLANES):
                if code == 0 and beyond[k].all() and not cov.any():
                    seen.add(f"outside_within_margin_{name}")      # kept by the cull, every corner beyond the plane in fp32
                if k < 4 and code == 0 and edge[k].any() and not beyond[k].any():
                    seen.add(f"visible_at_{name}")
        if ntri in (255, 256, 257) and cov.any():
            dw = st["depth"][cov]
            if (dw >= mo.DEPTH_MAX - 16).all():
                seen.add("block_on_far_plane")
            if (dw <= 16).all():
                seen.add("block_on_near_plane")
        if cov.any():
            with np.errstate(all="ignore"):
                rho2, lam = st["rho2"][cov], st["lam"][cov]
                if (rho2 <= 1).any():
                    seen.add("magnified")
                if (rho2 > 1).any():
                    seen.add("minified")
                # (rho2 is a sum of squares; with one term, the square of 1 -+ one step is 1 -+ two steps: the nearest it comes to 1)
                if (rho2 == 1).any():
                    seen.add("rho2_one")
                if ((rho2 > 1) & (rho2 <= f32(1 + 2.0 ** -22))).any():
                    seen.add("rho2_above_one")
                if ((rho2 < 1) & (rho2 >= f32(1 - 2.0 ** -23))).any():
                    seen.add("rho2_below_one")
                if ((rho2 > 1) & (lam == np.floor(lam)) & (lam >= 1)).any():
                    seen.add("integer_lambda")
                if ((rho2 > 1) & (st["l0"][cov] == st["l1"][cov])).any():
                    seen.add("top_level")
                if (st["grey"][cov] == 255).any():
                    seen.add("grey_255_covered")
                if (st["grey"][cov] == 0).any():
                    seen.add("grey_0")
                if np.isnan(st["luma"][cov]).any():
                    seen.add("nan_luma")
                u, v = st["u"][cov], st["v"][cov]
                lw, lh = levels[0].shape[1], levels[0].shape[0]
                x, y = u * f32(lw) - f32(0.5), v * f32(lh) - f32(0.5)
                for g in (x, y):
                    near = np.abs(g - np.rint(g)) <= 2 * np.spacing(np.abs(g))
                    if (g == np.rint(g)).any():
                        seen.add("texel_border")         # u w - 0.5 a whole number: the floor's decision
                    if (near & (g != np.rint(g))).any():
                        seen.add("texel_border_step")
                if ((np.floor(x) < 0) | (np.floor(x) >= lw - 1) | (np.floor(y) < 0) | (np.floor(y) >= lh - 1)).any():
                    seen.add("wrap_path")
                if ((np.abs(x) >= 2.0 ** 24 - lw) | (np.abs(y) >= 2.0 ** 24 - lh)).any():
                    seen.add("beyond_wrap_domain")
                    l0 = st["l0"][cov]
                    if any(levels[int(l)].shape[1] & (levels[int(l)].shape[1] - 1) or levels[int(l)].shape[0] & (levels[int(l)].shape[0] - 1)
                           for l in np.unique(l0)):
                        seen.add("odd_level")
            # the three reciprocals of the winners' shading
            for i in np.unique(st["piece_index"][cov]):
                p = st["pieces"][int(i)]
                yy, xx = np.nonzero(st["piece_index"] == i)
                sh = mo.shade(p["t"], p["tu"], p["tv"], levels, xx, yy)
                ok = np.ones(len(xx), bool)
                for q in (sh["Q"], sh["Qx"], sh["Qy"]):
                    e = _exp_field(q)
                    ok &= (e >= 3) & (e <= 252)
                seen.add("rcp_fast" if ok.any() else "rcp_division")
                if (~ok).any():
                    seen.add("rcp_division")
                with np.errstate(all="ignore"):
                    if ((sh["Q"] > 0) & ((sh["Qx"] <= 0) | (sh["Qy"] <= 0))).any():
                        seen.add("neighbour_beyond_horizon")
    return seen


def reached(cases, W, H):
    seen = set()
    for c in cases:
        seen |= branches(c, W, H)
    return seen
