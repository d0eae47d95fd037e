"""numpy (fp32) restatement of the textured-mesh render-stack producer -- TEST INFRASTRUCTURE ONLY.

Restates Rendering<1>::renderToTextureOnGPU (Thirdparty/Localization/rendering.hpp:530-630), the shaders
ShadingWithTexture.* (luma 0.299/0.587/0.114 of the texture sample) and the texture state of loadBMP_custom
(texture.cpp:31-96: GL_REPEAT, GL_LINEAR, GL_LINEAR_MIPMAP_LINEAR, glGenerateMipmap) with the OpenGL 3.3 specification's
rules in fp32: pixel centres at +0.5, top-left fill rule, back-face culling (front = counter-clockwise), perspective-
correct attributes (u/w, v/w, 1/w as planes over the window, one reciprocal per sample point), visibility by 24-bit depth
with GL_LESS (among equal depths the triangle drawn first), isotropic LOD from per-pixel uv differences, 2x2-box mip levels
rounded to RGB8, and clipping of
triangles against the near plane in clip space (GL clips primitives to the view volume before the perspective divide:
implied by glEnable(GL_DEPTH_TEST) / glDrawArrays(GL_TRIANGLES), rendering.hpp:294-300,619): Sutherland-Hodgman on
z_clip >= -w_clip, new corners interpolated from the inside corner towards the outside one.
"PARITY UNPINNED": an OpenGL driver rasterises in fixed point and may approximate the LOD; nothing to compare against.
Slow (python loop over triangles): small test meshes only.

The rule is written once, in stages, over a float type F: clip_coords -> _clip_near -> setup -> cover -> shade -> resolve
(render_staged).  F = float32 is the twin of csrc/nmi_mesh.hip (same operations in the same order, the device's conversions:
float -> int saturates and NaN converts to 0, fminf / fmaxf drop a NaN operand, GL_REPEAT by the kernel's fp32 wrap_index);
F = float64 is the MODEL (render_mesh_f64): every operation in float64 on the fp32 inputs, log2 in float64, GL_REPEAT by an
exact modulo.  render_mesh / render_stack return the twin's bytes.
"""
import numpy as np

f32 = np.float32
DEPTH_MAX = 0xFFFFFF
EMPTY_DEPTH = 1 << 24      # the depth of a pixel no fragment reached
SETUP_STATUS = ("kept", "cw", "plane", "area", "box")   # kept, or the first test that dropped the piece (tri_setup's order)


def sat_int(x):
    """float -> int32 as the device converts: towards zero, saturating, NaN -> 0 (numpy's astype is undefined there)."""
    x = np.asarray(x, np.float64)
    with np.errstate(invalid="ignore"):
        y = np.where(np.isnan(x), 0.0, np.clip(np.trunc(x), -2.0 ** 31, 2.0 ** 31 - 1))
    return y.astype(np.int64)


def sat_uint(x):
    """float -> uint32 likewise: negative and NaN -> 0, saturating at 2^32 - 1."""
    x = np.asarray(x, np.float64)
    with np.errstate(invalid="ignore"):
        y = np.where(np.isnan(x), 0.0, np.clip(np.trunc(x), 0.0, 2.0 ** 32 - 1))
    return y.astype(np.int64)


def wrap_index(x, n, bounded=True):
    """wrap_index of nmi_mesh.hip in fp32: x mod n for an integer-valued x, exact for |x| < 2^24 - n; beyond that clamped into
    [0, n - 1] (bounded=False: the rule before the clamp, kept for the test that shows what it did)."""
    x = np.asarray(x, f32)
    n = f32(n)
    inv = f32(1.0) / n
    with np.errstate(all="ignore"):
        r = x - np.floor(x * inv) * n
        r = np.where(r < 0, r + n, r)
        r = np.where(r >= n, r - n, r)
        if bounded:
            r = np.fmin(np.fmax(r, f32(0.0)), n - f32(1.0))
    return sat_int(r)


def mip_luma(rgb):
    """-> list of float32 luma levels (row 0 = v 0), mip chain by 2x2 box on RGB8 with rounding, like nmi_texture_create."""
    cur = np.ascontiguousarray(rgb, np.uint8)
    levels = []
    while True:
        c = cur.astype(f32) / f32(255.0)
        levels.append((f32(0.299) * c[..., 0] + f32(0.587) * c[..., 1]) + f32(0.114) * c[..., 2])
        h, w = cur.shape[:2]
        if (w == 1 and h == 1) or len(levels) == 16:
            break
        nw, nh = max(1, w // 2), max(1, h // 2)
        x0 = np.minimum(2 * np.arange(nw), w - 1)
        x1 = np.minimum(2 * np.arange(nw) + 1, w - 1)
        y0 = np.minimum(2 * np.arange(nh), h - 1)
        y1 = np.minimum(2 * np.arange(nh) + 1, h - 1)
        s = (cur[np.ix_(y0, x0)].astype(np.int32) + cur[np.ix_(y0, x1)] + cur[np.ix_(y1, x0)] + cur[np.ix_(y1, x1)])
        cur = ((s + 2) // 4).astype(np.uint8)
    return levels


def _repeat(xf, n, F):
    if F is f32:
        return wrap_index(xf, n)
    with np.errstate(invalid="ignore"):
        return np.where(np.isfinite(xf), np.mod(xf, F(n)), 0.0).astype(np.int64)   # (fmod is exact)


def _bilinear(level, u, v, F=f32):
    h, w = level.shape
    with np.errstate(all="ignore"):
        x = u * F(w) - F(0.5)
        y = v * F(h) - F(0.5)
        xf, yf = np.floor(x), np.floor(y)
        fx, fy = x - xf, y - yf
        i0, j0 = _repeat(xf, w, F), _repeat(yf, h, F)
        i1 = np.where(i0 + 1 == w, 0, i0 + 1)
        j1 = np.where(j0 + 1 == h, 0, j0 + 1)
        lv = level if F is f32 else level.astype(F)
        t00, t10, t01, t11 = lv[j0, i0], lv[j0, i1], lv[j1, i0], lv[j1, i1]
        a = t00 + (t10 - t00) * fx
        b = t01 + (t11 - t01) * fx
        return a + (b - a) * fy


def clip_coords(xyz, mvp_colmajor, F=f32):
    """-> cx, cy, cz, cw [T, 3]: glm mat4 * vec4 per corner, (m0 x + m1 y) + (m2 z + m3)."""
    m = np.asarray(mvp_colmajor, f32).astype(F)
    P = np.asarray(xyz, f32).reshape(-1, 3, 3).astype(F)
    x, y, z = P[..., 0], P[..., 1], P[..., 2]
    with np.errstate(all="ignore"):
        return tuple((m[r] * x + m[4 + r] * y) + (m[8 + r] * z + m[12 + r]) for r in range(4))


def _clip_near(cx, cy, cz, cw, tu, tv):
    """Near-plane clipping of one triangle in clip space -> list of 0, 1 or 2 triangles, each (cx, cy, cz, cw, tu, tv) of 3."""
    F = cx.dtype.type
    with np.errstate(all="ignore"):
        d = cz + cw
        inside = d >= 0
        n_in = int(inside.sum())
        if n_in == 0:
            return []
        if n_in == 3:
            return [(cx, cy, cz, cw, tu, tv)]
        poly = []
        for k in range(3):
            b = (k + 1) % 3
            if inside[k]:
                poly.append((cx[k], cy[k], cz[k], cw[k], tu[k], tv[k]))
            if inside[k] != inside[b]:
                i, o = (k, b) if inside[k] else (b, k)   # from the inside corner towards the outside one
                t = d[i] / (d[i] - d[o])
                w = cw[i] + (cw[o] - cw[i]) * t
                poly.append((cx[i] + (cx[o] - cx[i]) * t, cy[i] + (cy[o] - cy[i]) * t, -w, w, tu[i] + (tu[o] - tu[i]) * t,
                             tv[i] + (tv[o] - tv[i]) * t))
    out = []
    for a_, b_, c_ in ((0, 1, 2), (0, 2, 3))[:len(poly) - 2]:
        out.append(tuple(np.array([poly[a_][j], poly[b_][j], poly[c_][j]], F) for j in range(6)))
    return out


def setup(width, height, cx, cy, cz, cw):
    """tri_setup for one piece -> dict with status (SETUP_STATUS) and, when kept, the window corners xw / yw / zw, iw = 1 / cw, area,
    inv_area, the edges ex / ey (edge k opposite corner k) with their ownership, and the pixel box x_lo .. y_hi."""
    F = cx.dtype.type
    with np.errstate(all="ignore"):
        if not (cw > 0).all():
            return {"status": "cw"}
        if ((cx < -cw).all() or (cx > cw).all() or (cy < -cw).all() or (cy > cw).all() or (cz < -cw).all() or (cz > cw).all()):
            return {"status": "plane"}
        xw = (cx / cw * F(0.5) + F(0.5)) * F(width)
        yw = (cy / cw * F(0.5) + F(0.5)) * F(height)
        zw = cz / cw * F(0.5) + F(0.5)
        iw = F(1.0) / cw
        area = (xw[1] - xw[0]) * (yw[2] - yw[0]) - (xw[2] - xw[0]) * (yw[1] - yw[0])
        t = {"status": "area", "xw": xw, "yw": yw, "zw": zw, "iw": iw, "area": area}
        if not area > 0:
            return t
        # (fminf / fmaxf: a NaN operand is dropped; no corner is NaN here, the area would be)
        x_lo = max(0, int(sat_int(np.ceil(np.fmin.reduce(xw) - F(0.5)))))
        x_hi = min(width - 1, int(sat_int(np.floor(np.fmax.reduce(xw) - F(0.5)))))
        y_lo = max(0, int(sat_int(np.ceil(np.fmin.reduce(yw) - F(0.5)))))
        y_hi = min(height - 1, int(sat_int(np.floor(np.fmax.reduce(yw) - F(0.5)))))
        t.update(status="box", x_lo=x_lo, x_hi=x_hi, y_lo=y_lo, y_hi=y_hi)
        if x_lo > x_hi or y_lo > y_hi:
            return t
        ex = np.array([xw[(k + 2) % 3] - xw[(k + 1) % 3] for k in range(3)], F)
        ey = np.array([yw[(k + 2) % 3] - yw[(k + 1) % 3] for k in range(3)], F)
        own = [bool(ey[k] < 0 or (ey[k] == 0 and ex[k] < 0)) for k in range(3)]
        t.update(status="kept", ex=ex, ey=ey, own=own, inv_area=F(1.0) / area)
    return t


def _weights(t, px, py):
    xw, yw, ex, ey, inv_area = t["xw"], t["yw"], t["ex"], t["ey"], t["inv_area"]
    with np.errstate(all="ignore"):
        return [(ex[k] * (py - yw[(k + 1) % 3]) - ey[k] * (px - xw[(k + 1) % 3])) * inv_area for k in range(3)]


def cover(t, region=None):
    """tri_cover over the piece's box, or over region = (x_lo, x_hi, y_lo, y_hi) (pixels outside the piece's own box are not
    inside) -> dict: xx, yy, the three edge values b (barycentric weights), inside, z, depth (24 bits)."""
    F = t["xw"].dtype.type
    x_lo, x_hi, y_lo, y_hi = region if region is not None else (t["x_lo"], t["x_hi"], t["y_lo"], t["y_hi"])
    yy, xx = np.mgrid[y_lo:y_hi + 1, x_lo:x_hi + 1]
    fxp = xx.astype(F) + F(0.5)
    fyp = yy.astype(F) + F(0.5)
    b = _weights(t, fxp, fyp)
    zw = t["zw"]
    with np.errstate(all="ignore"):
        zz = (b[0] * zw[0] + b[1] * zw[1]) + b[2] * zw[2]
        inside = (xx >= t["x_lo"]) & (xx <= t["x_hi"]) & (yy >= t["y_lo"]) & (yy <= t["y_hi"])
        for k in range(3):
            inside &= (b[k] > 0) | ((b[k] == 0) & t["own"][k])
        inside &= (zz >= 0) & (zz <= 1)
        depth = np.minimum(sat_uint(zz * F(16777215.0) + F(0.5)), DEPTH_MAX)
    return {"xx": xx, "yy": yy, "b": b, "inside": inside, "z": zz, "depth": depth}


def planes(t, tu, tv):
    """tri_planes: S = u/w, R = v/w, Q = 1/w as (value at the centre of the box's first pixel, d/dx, d/dy)."""
    F = t["xw"].dtype.type
    ex, ey, inv_area, iw = t["ex"], t["ey"], t["inv_area"], t["iw"]
    xr, yr = F(t["x_lo"]) + F(0.5), F(t["y_lo"]) + F(0.5)
    with np.errstate(all="ignore"):
        b0 = _weights(t, xr, yr)
        bx = [(-ey[k]) * inv_area for k in range(3)]
        by = [ex[k] * inv_area for k in range(3)]
        sc = [tu[k] * iw[k] for k in range(3)]
        rc = [tv[k] * iw[k] for k in range(3)]

        def plane(g):
            return ((b0[0] * g[0] + b0[1] * g[1]) + b0[2] * g[2], (bx[0] * g[0] + bx[1] * g[1]) + bx[2] * g[2],
                    (by[0] * g[0] + by[1] * g[1]) + by[2] * g[2])

        return xr, yr, plane(sc), plane(rc), plane(iw)


def shade(t, tu, tv, levels, xx, yy):
    """shade_pixel at the pixels (xx, yy) of a kept piece -> dict: u, v, Q, Qx, Qy, rho2, lam (lambda; meaningful where rho2 > 1),
    l0, l1 (the level pair; 0, 0 when magnified), s0, s1 (the two levels' samples) and f (the blend), luma = s0 + (s1 - s0) f (before
    clamping and rounding), grey."""
    F = t["xw"].dtype.type
    tw, th = F(levels[0].shape[1]), F(levels[0].shape[0])
    nlev = len(levels)
    xr, yr, (s0, sx, sy), (r0, rx, ry), (q0, qx, qy) = planes(t, tu, tv)
    fxp = np.asarray(xx).astype(F) + F(0.5)
    fyp = np.asarray(yy).astype(F) + F(0.5)
    with np.errstate(all="ignore"):
        dx, dy = fxp - xr, fyp - yr
        S = (s0 + sx * dx) + sy * dy
        R = (r0 + rx * dx) + ry * dy
        Q = (q0 + qx * dx) + qy * dy
        Qx, Qy = Q + qx, Q + qy
        iq, iqx, iqy = F(1.0) / Q, F(1.0) / Qx, F(1.0) / Qy     # (warp_rcp_fast gives the division's bits)
        u, v = S * iq, R * iq
        ux, vx = (S + sx) * iqx, (R + rx) * iqx
        uy, vy = (S + sy) * iqy, (R + ry) * iqy
        dudx, dvdx, dudy, dvdy = (ux - u) * tw, (vx - v) * th, (uy - u) * tw, (vy - v) * th
        rho2 = np.fmax(dudx * dudx + dvdx * dvdx, dudy * dudy + dvdy * dvdy)   # fmaxf: a NaN operand is dropped
        mini = rho2 > 1                                     # false for NaN: the magnification branch
        lam = F(0.5) * np.log2(np.where(mini, rho2, F(1.0))).astype(F)   # log2 of the longer footprint axis = half the log2 of its square
        luma = _bilinear(levels[0], u, v, F)
        l0 = np.zeros(np.shape(luma), np.int64)
        l1 = l0.copy()
        s0_, s1_, fr = luma, luma, np.zeros(np.shape(luma), F)
        if mini.any():
            lc = np.fmin(np.fmax(lam, F(0.0)), F(nlev - 1))
            l0 = np.where(mini, sat_int(np.floor(lc)), 0)
            l1 = np.where(mini, np.minimum(l0 + 1, nlev - 1), 0)
            fr = lc - l0.astype(F)
            for L in np.unique(l0[mini]):
                sel = mini & (l0 == L)
                a = _bilinear(levels[int(L)], u, v, F)
                b = _bilinear(levels[min(int(L) + 1, nlev - 1)], u, v, F)
                luma = np.where(sel, a + (b - a) * fr, luma)
                s0_, s1_ = np.where(sel, a, s0_), np.where(sel, b, s1_)
            fr = np.where(mini, fr, F(0.0))
        grey = sat_uint(np.fmin(np.fmax(luma, F(0.0)), F(1.0)) * F(255.0) + F(0.5))   # fminf(fmaxf(NaN, 0), 1) = 0
    return {"u": u, "v": v, "Q": Q, "Qx": Qx, "Qy": Qy, "rho2": rho2, "lam": lam, "l0": l0, "l1": l1, "s0": s0_, "s1": s1_, "f": fr,
            "luma": luma, "grey": grey}


def pieces(xyz, uv, mvp_colmajor, width, height, F=f32):
    """Every (triangle, piece) of one view in draw order -> list of dicts: tri, piece, tu, tv, d (the triangle's near-plane
    distances), n_in, and the set-up result (setup)."""
    cx, cy, cz, cw = clip_coords(xyz, mvp_colmajor, F)
    T = np.asarray(uv, f32).reshape(-1, 3, 2).astype(F)
    out = []
    for tri in range(cx.shape[0]):
        with np.errstate(all="ignore"):
            d = cz[tri] + cw[tri]
        n_in = int((d >= 0).sum())
        for sub, c in enumerate(_clip_near(cx[tri], cy[tri], cz[tri], cw[tri], T[tri, :, 0], T[tri, :, 1])):
            t = setup(width, height, *c[:4])
            out.append({"tri": tri, "piece": sub, "tu": c[4], "tv": c[5], "clip": c[:4], "d": d, "n_in": n_in, "t": t})
    return out


def render_staged(xyz, uv, levels, mvp_colmajor, width, height, F=f32, keep_cover=False):
    """One view, every stage kept -> dict: pieces (see pieces(); with keep_cover each kept piece's cover() as "cover"), and per
    pixel [H, W]: nfrag (fragments that passed coverage and the depth clip), tri / piece (the winner; -1: none), depth
    (EMPTY_DEPTH: none), and the winner's u, v, rho2, lam, l0, l1, s0, s1, f, luma, grey (255 where no fragment won)."""
    ps = pieces(xyz, uv, mvp_colmajor, width, height, F)
    depth = np.full((height, width), EMPTY_DEPTH, np.int64)
    tri = np.full((height, width), -1, np.int64)
    piece = np.full((height, width), -1, np.int64)
    nfrag = np.zeros((height, width), np.int64)
    for i, p in enumerate(ps):
        t = p["t"]
        if t["status"] != "kept":
            continue
        c = cover(t)
        if keep_cover:
            p["cover"] = c
        if not c["inside"].any():
            continue
        box = (slice(t["y_lo"], t["y_hi"] + 1), slice(t["x_lo"], t["x_hi"] + 1))
        nfrag[box] += c["inside"]
        # GL_LESS keeps the fragment drawn first among equal depths, and pieces arrive in draw order: a fragment wins only with
        # a strictly smaller depth (the key depth << 40 | triangle << 10 | piece << 9 | slot of nmi_mesh.hip)
        win = c["inside"] & (c["depth"] < depth[box])
        depth[box] = np.where(win, c["depth"], depth[box])
        tri[box] = np.where(win, p["tri"], tri[box])
        piece[box] = np.where(win, i, piece[box])      # (index into ps for now)
    out = {k: np.full((height, width), np.nan, F) for k in ("u", "v", "rho2", "lam", "luma", "s0", "s1", "f")}
    out.update({k: np.zeros((height, width), np.int64) for k in ("l0", "l1")})
    grey = np.full((height, width), 255, np.int64)
    for i in np.unique(piece[piece >= 0]):
        p = ps[int(i)]
        yy, xx = np.nonzero(piece == i)
        s = shade(p["t"], p["tu"], p["tv"], levels, xx, yy)
        for k in out:
            out[k][yy, xx] = s[k]
        grey[yy, xx] = s["grey"]
    sub = np.array([p["piece"] for p in ps] + [-1], np.int64)
    out.update(pieces=ps, nfrag=nfrag, tri=tri, piece=sub[piece], piece_index=piece, depth=depth, grey=grey.astype(np.uint8),
               covered=tri >= 0)
    return out


def render_mesh_f64(xyz, uv, levels, mvp_colmajor, width, height, keep_cover=False):
    """The float64 model of the same rule: render_staged with every operation in float64 on the fp32 inputs."""
    return render_staged(xyz, uv, levels, mvp_colmajor, width, height, np.float64, keep_cover)


def render_mesh(xyz, uv, levels, mvp_colmajor, width, height):
    """One view -> uint8 [H, W], bottom-up rows, background 255."""
    return render_staged(xyz, uv, levels, mvp_colmajor, width, height)["grey"]


def _raster(zbuf, levels, width, height, cx, cy, cz, cw, tu, tv):
    """One piece into zbuf (uint64 [H, W]: depth << 8 | grey; empty 0xFFFFFFFFFF), as render_staged resolves it."""
    t = setup(width, height, cx, cy, cz, cw)
    if t["status"] != "kept":
        return
    c = cover(t)
    sub = zbuf[t["y_lo"]:t["y_hi"] + 1, t["x_lo"]:t["x_hi"] + 1]
    win = c["inside"] & (c["depth"].astype(np.uint64) < (sub >> np.uint64(8)))
    if not win.any():
        return
    grey = shade(t, tu, tv, levels, c["xx"][win], c["yy"][win])["grey"]
    sub[win] = (c["depth"][win].astype(np.uint64) << np.uint64(8)) | grey.astype(np.uint64)


def render_stack(xyz, uv, levels, mvps, width, height):
    return np.stack([render_mesh(xyz, uv, levels, m, width, height) for m in np.asarray(mvps, f32).reshape(-1, 16)])
