"""Derived fp32 error bounds for the mesh rule, and the twin-vs-float64-model comparison built on them -- TEST INFRASTRUCTURE ONLY.

Ev is a float64 value with a bound on |fp32 value - float64 value|, carried through the twin's own sequence of operations by the
standard model of rounding: fl(a o b) = (a o b)(1 + d), |d| <= u = 2^-24 (or an absolute 2^-149 where the result is
subnormal).  If the operands are off by ea, eb, the exact result of the fp32 operands is off by
    P(+, -) = ea + eb,    P(*) = |a| eb + |b| ea + ea eb,    P(/) = (ea + |a / b| eb) / (|b| - eb)   (inf when |b| <= eb),
and the rounded one by P + u (|a o b| + P) + 2^-149.  A product or quotient with an error-free power of two (1 / 2, cw = 1) does not
round at all.  max(a, b) is off by max(ea, eb).  A bound that reaches 2^127 is inf (the
fp32 value may overflow).  Nothing here is fitted to what the twin gives: tests/test_mesh_edges.py::test_bound_holds checks
every bound against the twin.

compare_view() applies the criterion of tests/test_mesh_edges.py's docstring to one view.
"""
import numpy as np

from oracle import mesh_oracle_np as mo

f32 = np.float32
U = 2.0 ** -24
TINY = 2.0 ** -149
D = float(mo.DEPTH_MAX)


class Ev:
    __slots__ = ("v", "e")

    def __init__(self, v, e=0.0):
        self.v = np.asarray(v, np.float64)
        self.e = np.asarray(e, np.float64)

    @staticmethod
    def _round(v, p):
        with np.errstate(all="ignore"):
            e = p + U * (np.abs(v) + p) * (1 + 1e-9) + TINY
            return Ev(v, np.where(np.isfinite(e) & (np.abs(v) + e < 2.0 ** 127), e, np.inf))

    @staticmethod
    def _pow2(o):
        with np.errstate(all="ignore"):
            m, _ = np.frexp(np.abs(o.v))
            return (o.e == 0) & (m == 0.5) & (np.abs(o.v) > 2.0 ** -100) & (np.abs(o.v) < 2.0 ** 100)

    @staticmethod
    def of(x):
        return x if isinstance(x, Ev) else Ev(x)

    def __add__(self, o):
        o = Ev.of(o)
        with np.errstate(all="ignore"):
            return Ev._round(self.v + o.v, self.e + o.e)

    def __sub__(self, o):
        o = Ev.of(o)
        with np.errstate(all="ignore"):
            return Ev._round(self.v - o.v, self.e + o.e)

    def __mul__(self, o):
        o = Ev.of(o)
        with np.errstate(all="ignore"):
            # (0 * inf: an operand that is exactly 0 with no error contributes nothing)
            p = np.where(self.e == 0, 0.0, np.abs(o.v) * self.e) + np.where(o.e == 0, 0.0, np.abs(self.v) * o.e) + \
                np.where((self.e == 0) | (o.e == 0), 0.0, self.e * o.e)
            r = Ev._round(self.v * o.v, p)
            exact = Ev._pow2(o) | Ev._pow2(self)       # scaling by a power of two: no rounding (the result stays normal: checked below)
            ok = exact & (np.abs(r.v) > 2.0 ** -100) & (np.abs(r.v) < 2.0 ** 100) & np.isfinite(r.e)
            return Ev(r.v, np.where(ok, p, r.e))

    def __truediv__(self, o):
        o = Ev.of(o)
        with np.errstate(all="ignore"):
            z = self.v / o.v
            den = np.abs(o.v) - o.e
            p = np.where(den > 0, (self.e + np.abs(z) * o.e) / np.where(den > 0, den, 1.0), np.inf)
            r = Ev._round(z, p)
            ok = Ev._pow2(o) & (np.abs(r.v) > 2.0 ** -100) & (np.abs(r.v) < 2.0 ** 100) & np.isfinite(r.e)
            return Ev(r.v, np.where(ok, p, r.e))

    def __neg__(self):
        return Ev(-self.v, self.e)

    def __getitem__(self, k):
        return Ev(self.v[k], self.e[k] if self.e.ndim else self.e)

    def near(self, x=0.0):
        """True where the decision "value vs x" is within the bound (or the bound is not finite)."""
        with np.errstate(all="ignore"):
            return ~(np.abs(self.v - x) > self.e)


def ev_max(a, b):
    return Ev(np.fmax(a.v, b.v), np.fmax(a.e, b.e))


def ev_stack(lst):
    return Ev(np.stack([np.broadcast_to(x.v, np.broadcast(x.v, x.e).shape) for x in lst]),
              np.stack([np.broadcast_to(x.e, np.broadcast(x.v, x.e).shape) for x in lst]))


def clip_ev(P3, m):
    """Clip coordinates of three corners P3 [3, 3] (fp32 values) -> [cx, cy, cz, cw] as Ev [3], each within E_r = 3u T_r,
    T_r = sum_j |m_rj p_j| + |m_r3| (a 4-term sum of rounded products: four roundings of terms, three of partial sums no larger than T)."""
    M = np.asarray(m, f32).astype(np.float64).reshape(4, 4).T
    P = np.asarray(P3, f32).astype(np.float64).reshape(3, 3)
    with np.errstate(all="ignore"):
        c = P @ M[:, :3].T + M[:, 3]
        T = np.abs(P) @ np.abs(M[:, :3]).T + np.abs(M[:, 3])
        E = 3 * U * T * (1 + 1e-6) + 4 * TINY
        E = np.where(np.isfinite(T) & (T < 2.0 ** 127) & np.isfinite(c), E, np.inf)
        # a row with ONE nonzero entry that is a power of two (the EXACT matrix of the cases: cx = x, ..., cw = 1) rounds nothing:
        # the other products are 0 exactly, the sums add 0, the product scales by a power of two
        Mr = np.c_[M[:, :3], M[:, 3]]
        m_, _ = np.frexp(np.abs(Mr))
        one = ((Mr != 0).sum(1) == 1) & ((m_ == 0.5) | (Mr == 0)).all(1)
        E = np.where(one[None, :] & np.isfinite(E) & (np.abs(c) > 2.0 ** -100), 0.0, E)
    return [Ev(c[:, r], E[:, r]) for r in range(4)]


def clip_poly_ev(c, tu, tv, inside):
    """_clip_near's polygon for the corner pattern `inside` (1 or 2 true) -> list of pieces, each ([cx, cy, cz, cw] Ev [3], tu, tv Ev [3])."""
    cx, cy, cz, cw = c
    d = cz + cw
    tu, tv = Ev(np.asarray(tu, np.float64)), Ev(np.asarray(tv, np.float64))
    poly = []
    for k in range(3):
        b = (k + 1) % 3
        if inside[k]:
            poly.append((cx[k], cy[k], cz[k], cw[k], tu[k], tv[k]))
        if inside[k] != inside[b]:
            i, o = (k, b) if inside[k] else (b, k)
            t = d[i] / (d[i] - d[o])
            w = cw[i] + (cw[o] - cw[i]) * t
            poly.append((cx[i] + (cx[o] - cx[i]) * t, cy[i] + (cy[o] - cy[i]) * t, -w, w, tu[i] + (tu[o] - tu[i]) * t,
                         tv[i] + (tv[o] - tv[i]) * t))
    out = []
    for a_, b_, c_ in ((0, 1, 2), (0, 2, 3))[:len(poly) - 2]:
        cols = [ev_stack([poly[a_][j], poly[b_][j], poly[c_][j]]) for j in range(6)]
        out.append((cols[:4], cols[4], cols[5]))
    return out


def setup_ev(c, W, H):
    """tri_setup's values for one piece -> dict of Ev: xw, yw, zw, iw [3], area, and the clip tests' robustness."""
    cx, cy, cz, cw = c
    xw = (cx / cw * 0.5 + 0.5) * float(W)
    yw = (cy / cw * 0.5 + 0.5) * float(H)
    zw = cz / cw * 0.5 + 0.5
    iw = Ev(1.0) / cw
    area = (xw[1] - xw[0]) * (yw[2] - yw[0]) - (xw[2] - xw[0]) * (yw[1] - yw[0])
    # "all three corners beyond plane p" is decided the same way in fp32 when one corner is inside by more than its bound, or all
    # are outside by more than theirs
    plane_ex = False
    for g in (cx, cy, cz):
        for s in (cw + g, cw - g):      # >= 0: inside
            robust = (s.v > s.e).any() or (s.v < -s.e).all()
            plane_ex |= not robust
    return {"xw": xw, "yw": yw, "zw": zw, "iw": iw, "area": area, "cw_ex": bool(cw.near(0).any()), "plane_ex": bool(plane_ex),
            "area_ex": bool(area.near(0))}


def box_robust(s, W, H):
    """The pixel box's four bounds are the same in fp32: min / max of the window coordinates farther than their bound from the
    rounding decision (an integer + 1/2), or clamped by the window on both sides of it."""
    ok = True
    for g, n in ((s["xw"], W), (s["yw"], H)):
        for v, e in ((np.min(g.v - 0.5), np.max(g.e)), (np.max(g.v - 0.5), np.max(g.e))):
            if not np.isfinite(e) or not np.isfinite(v):
                return False
            if v + e < -1 or v - e > n:      # clamped to the window whatever the rounding
                continue
            ok &= abs(v - np.rint(v)) > e + U * (abs(v) + 1)    # (the - 0.5 itself rounds)
    return bool(ok)


def edges_ev(s):
    xw, yw = s["xw"], s["yw"]
    ex = [xw[(k + 2) % 3] - xw[(k + 1) % 3] for k in range(3)]
    ey = [yw[(k + 2) % 3] - yw[(k + 1) % 3] for k in range(3)]
    return ex, ey, Ev(1.0) / s["area"]


def weights_ev(s, px, py):
    ex, ey, inv_area = edges_ev(s)
    xw, yw = s["xw"], s["yw"]
    px, py = Ev(px), Ev(py)
    return [(ex[k] * (py - yw[(k + 1) % 3]) - ey[k] * (px - xw[(k + 1) % 3])) * inv_area for k in range(3)]


def cover_ev(s, xx, yy):
    """-> (b: three Ev, z: Ev, derr: the depth's bound in steps) at the pixels (xx, yy)."""
    b = weights_ev(s, xx + 0.5, yy + 0.5)
    zw = s["zw"]
    z = (b[0] * zw[0] + b[1] * zw[1]) + b[2] * zw[2]
    # round(z (2^24 - 1)) in fp32: the product and the + 0.5 each round at a spacing of at most 1
    with np.errstate(all="ignore"):
        derr = np.ceil(z.e * D + 2)
    return b, z, derr


def shade_ev(s, tu, tv, x_lo, y_lo, xx, yy, tw, th):
    """shade_pixel's u, v, rho2 and lambda as Ev at the pixels (xx, yy), planes about the centre of pixel (x_lo, y_lo)."""
    ex, ey, inv_area = edges_ev(s)
    iw = s["iw"]
    xr, yr = x_lo + 0.5, y_lo + 0.5
    b0 = weights_ev(s, xr, yr)
    bx = [(-ey[k]) * inv_area for k in range(3)]
    by = [ex[k] * inv_area for k in range(3)]
    sc = [tu[k] * iw[k] for k in range(3)]
    rc = [tv[k] * iw[k] for k in range(3)]
    iwl = [iw[k] for k in range(3)]

    def plane(g):
        return ((b0[0] * g[0] + b0[1] * g[1]) + b0[2] * g[2], (bx[0] * g[0] + bx[1] * g[1]) + bx[2] * g[2],
                (by[0] * g[0] + by[1] * g[1]) + by[2] * g[2])

    (s0, sx, sy), (r0, rx, ry), (q0, qx, qy) = plane(sc), plane(rc), plane(iwl)
    dx, dy = Ev(xx + 0.5 - xr), Ev(yy + 0.5 - yr)
    S = (s0 + sx * dx) + sy * dy
    R = (r0 + rx * dx) + ry * dy
    Q = (q0 + qx * dx) + qy * dy
    iq, iqx, iqy = Ev(1.0) / Q, Ev(1.0) / (Q + qx), Ev(1.0) / (Q + qy)
    u, v = S * iq, R * iq
    ux, vx = (S + sx) * iqx, (R + rx) * iqx
    uy, vy = (S + sy) * iqy, (R + ry) * iqy
    dudx, dvdx, dudy, dvdy = (ux - u) * tw, (vx - v) * th, (uy - u) * tw, (vy - v) * th
    rho2 = ev_max(dudx * dudx + dvdx * dvdx, dudy * dudy + dvdy * dvdy)
    with np.errstate(all="ignore"):
        # lambda = log2(rho2) / 2: d lambda <= d rho2 / (2 ln 2 (rho2 - d rho2)); log2f itself within 2 ulp of a value that is at
        # least 2^-24 in magnitude next to 1 (absolute 2^-22 covers both, relative 4u beyond)
        lam = 0.5 * np.log2(np.where(rho2.v > 0, rho2.v, 1.0))
        lo = rho2.v - rho2.e
        elam = np.where(lo > 0, rho2.e / (2 * np.log(2.0) * np.where(lo > 0, lo, 1.0)), np.inf) + 4 * U * np.abs(lam) + 2.0 ** -22
    return u, v, rho2, Ev(lam, elam)


def level_lipschitz(levels):
    """Per level: the largest |difference| of horizontally and of vertically adjacent texels, the wrap-around pair included --
    the Lipschitz constants of the GL_REPEAT bilinear sample in texel units."""
    out = []
    for lv in levels:
        a = lv.astype(np.float64)
        out.append((np.abs(a - np.roll(a, 1, 1)).max(), np.abs(a - np.roll(a, 1, 0)).max()))
    return out


def grey_bound(levels, lips, u, v, rho2, lam):
    """Bound on |luma(fp32) 255 - luma(model) 255| before rounding, from the bounds on u, v and lambda.

    The sampled luma is a continuous function of (u, v, lambda): bilinear within a level (continuous across texel borders and the
    repeat seam), linear in lambda between levels floor(lambda) and the next, continuous at integer lambda (f = 0 there), at
    lambda = 0 (the magnification branch samples level 0 alone) and at the clamp.  So
        |d luma| <= max over the levels in reach of (Lx_l w_l |du'| + Ly_l h_l |dv'|) + max |s_(l+1) - s_l| |d lambda| + 8u,
    with |du'| = |du| + 2u (|u| + 1 / w_l) for the rounding of x = u w - 0.5, Lx_l / Ly_l the level's largest neighbour differences,
    the s_l sampled by the model at this uv, the levels in reach those that lambda +- d lambda touches, and 8u for the three
    interpolations of each of two samples and their blend (values in [0, 1]).  Where d lambda is not finite the bound is 1."""
    n = len(levels)
    with np.errstate(all="ignore"):
        lam_lo = np.clip(np.where(rho2.v - rho2.e > 1, lam.v - lam.e, 0.0), 0, n - 1)
        lam_hi = np.clip(np.where(rho2.v + rho2.e > 1, lam.v + lam.e, 0.0), 0, n - 1)
        # (where rho2 + d rho2 <= 1 both sides magnify: lambda, whose bound is not finite next to rho2 = 0, plays no part)
        bad = (~np.isfinite(lam.e) & ~(rho2.v + rho2.e <= 1)) | ~np.isfinite(u.e) | ~np.isfinite(v.e)
        lam_lo, lam_hi = np.where(bad, 0, lam_lo), np.where(bad, 0, lam_hi)
        a, b = np.floor(lam_lo).astype(int), np.minimum(np.floor(lam_hi).astype(int) + 1, n - 1)
        g = np.zeros(u.v.shape)
        dl = np.zeros(u.v.shape)
        samples = [mo._bilinear(lv, u.v, v.v, np.float64) for lv in levels]
        for l in range(n):
            h, w = levels[l].shape
            reach = (a <= l) & (l <= b)
            du = u.e + 2 * U * (np.abs(u.v) + 1.0 / w)
            dv = v.e + 2 * U * (np.abs(v.v) + 1.0 / h)
            g = np.where(reach, np.maximum(g, lips[l][0] * w * du + lips[l][1] * h * dv), g)
            if l + 1 < n:
                dl = np.where(reach & (l + 1 <= b), np.maximum(dl, np.abs(samples[l + 1] - samples[l])), dl)
        width = lam_hi - lam_lo
        out = 255.0 * (g + dl * width + 8 * U)
        return np.where(bad | ~np.isfinite(out), 255.0, np.minimum(out, 255.0))


def compare_view(xyz, uv, levels, m, W, H, bulk=None, check_cover_bounds=True):
    """The criterion for one view.  -> dict: problems (list of strings: empty when the twin meets the model), bound_problems
    (a derived bound that the twin's value exceeds), frags / frags_exempt (fragments of bulk triangles), pixels / pixels_exempt,
    grey_pixels / grey_loose (bulk triangles' winning pixels compared in grey / those whose bound G is 1 or more),
    depth_decided_up / _down (fragments where rounding to nearest is decided, and which way),
    twin / model (the staged renders)."""
    T = mo.render_staged(xyz, uv, levels, m, W, H, f32, keep_cover=True)
    M = mo.render_staged(xyz, uv, levels, m, W, H, np.float64, keep_cover=True)
    P3 = np.asarray(xyz, f32).reshape(-1, 3, 3)
    UV = np.asarray(uv, f32).reshape(-1, 3, 2).astype(np.float64)
    ntri = len(P3)
    bulk = np.ones(ntri, bool) if bulk is None else np.asarray(bulk, bool)
    tw_pieces = {(p["tri"], p["piece"]): p for p in T["pieces"]}
    md_pieces = {(p["tri"], p["piece"]): p for p in M["pieces"]}
    c32 = [np.asarray(a, np.float64) for a in mo.clip_coords(xyz, m, f32)]
    problems, bound_problems = [], []
    px_exempt = np.zeros((H, W), bool)
    derr_win = np.zeros((H, W))
    frag_store = []
    n_frag = n_ex = 0
    n_decided = [0, 0]      # fragments whose depth rounding is decided: up, down
    n_grey = n_loose = 0    # common winners whose grey is compared / whose bound G is a whole grey level or more
    evs = {}

    def exempt_fragments(p):
        """Every fragment of a piece whose set-up is within a bound of a decision is exempt."""
        nonlocal n_frag, n_ex
        c = p.get("cover")
        if c is None or not c["inside"].any():
            return
        px_exempt[c["yy"][c["inside"]], c["xx"][c["inside"]]] = True
        if bulk[p["tri"]]:
            n_frag += int(c["inside"].sum())
            n_ex += int(c["inside"].sum())

    for tri in range(ntri):
        c = clip_ev(P3[tri], m)
        for r, name in enumerate("xyzw"):
            bad = ~(np.abs(c32[r][tri] - c[r].v) <= c[r].e)
            if (bad & np.isfinite(c[r].e)).any():
                bound_problems.append(f"tri {tri}: clip {name} off by {np.abs(c32[r][tri] - c[r].v).max():.3g} > {c[r].e.max():.3g}")
        d = c[2] + c[3]
        clip_ex = bool(d.near(0).any())
        in_m = d.v >= 0
        mine = [tw_pieces.get((tri, s)) for s in (0, 1)]
        theirs = [md_pieces.get((tri, s)) for s in (0, 1)]
        tw_d = np.asarray(mine[0]["d"] if mine[0] else c32[2][tri].astype(f32) + c32[3][tri].astype(f32), np.float64)
        same_pattern = bool(((tw_d >= 0) == in_m).all())
        if not same_pattern:
            if not clip_ex:
                problems.append(f"tri {tri}: corners inside the near plane differ: twin d {tw_d}, model {d.v}, bound {d.e}")
            for p in mine + theirs:
                if p:
                    exempt_fragments(p)
            continue
        n_in = int(in_m.sum())
        if n_in == 0:
            continue
        parts = [(c, Ev(UV[tri, :, 0]), Ev(UV[tri, :, 1]))] if n_in == 3 else clip_poly_ev(c, UV[tri, :, 0], UV[tri, :, 1], in_m)
        for sub, (cc, tu, tv) in enumerate(parts):
            pt, pm = mine[sub], theirs[sub]
            s = setup_ev(cc, W, H)
            st_t, st_m = pt["t"]["status"], pm["t"]["status"]
            # (a piece cut at the near plane has corners ON it, cz = -cw exactly in both; an original corner is inside it by more than
            # its bound, or the triangle is exempt as a whole, so that plane's test is no decision here)
            setup_ex = s["cw_ex"] or s["plane_ex"] or s["area_ex"]
            if st_t in ("kept", "box") and st_m in ("kept", "box"):
                boxes_equal = all(pt["t"][k] == pm["t"][k] for k in ("x_lo", "x_hi", "y_lo", "y_hi"))
                if not boxes_equal and box_robust(s, W, H) and not setup_ex:
                    problems.append(f"tri {tri}.{sub}: pixel boxes differ with robust bounds")
                if not boxes_equal:
                    setup_ex = True
            if st_t != st_m and not setup_ex:
                problems.append(f"tri {tri}.{sub}: set-up {st_t} (twin) vs {st_m} (model)")
            if st_t not in ("cw", "plane") and st_m not in ("cw", "plane") and np.isfinite(s["area"].e):
                for k in ("xw", "yw", "zw", "iw"):
                    bad = ~(np.abs(pt["t"][k].astype(np.float64) - s[k].v) <= s[k].e) & np.isfinite(s[k].e)
                    if bad.any():
                        bound_problems.append(f"tri {tri}.{sub}: {k} off by {np.abs(pt['t'][k] - s[k].v).max():.3g} > {s[k].e.max():.3g}")
                if not abs(float(pt["t"]["area"]) - s["area"].v) <= s["area"].e:
                    bound_problems.append(f"tri {tri}.{sub}: area off by {abs(float(pt['t']['area']) - s['area'].v):.3g} > {s['area'].e:.3g}")
            if st_t != "kept" or st_m != "kept" or setup_ex:
                for p in (pt, pm):
                    exempt_fragments(p)
                continue
            # ---- both kept, same box: coverage and depth per pixel of the box
            ct, cm = pt["cover"], pm["cover"]
            b, z, derr = cover_ev(s, ct["xx"].astype(np.float64), ct["yy"].astype(np.float64))
            with np.errstate(all="ignore"):
                fex = b[0].near(0) | b[1].near(0) | b[2].near(0) | z.near(0) | z.near(1) | ~np.isfinite(derr)
            if check_cover_bounds:
                for k in range(3):
                    bad = ~(np.abs(ct["b"][k].astype(np.float64) - b[k].v) <= b[k].e) & np.isfinite(b[k].e)
                    if bad.any():
                        bound_problems.append(f"tri {tri}.{sub}: edge value {k} off by more than its bound at {int(bad.sum())} pixels")
                bad = ~(np.abs(ct["z"].astype(np.float64) - z.v) <= z.e) & np.isfinite(z.e)
                if bad.any():
                    bound_problems.append(f"tri {tri}.{sub}: z off by more than its bound at {int(bad.sum())} pixels")
            diff = (ct["inside"] != cm["inside"]) & ~fex
            if diff.any():
                problems.append(f"tri {tri}.{sub}: coverage differs at {int(diff.sum())} pixels outside every bound")
            both = ct["inside"] & cm["inside"]
            bad = both & (np.abs(ct["depth"] - cm["depth"]) > derr)
            if bad.any():
                problems.append(f"tri {tri}.{sub}: depth beyond its bound at {int(bad.sum())} pixels "
                                f"(twin {ct['depth'][bad][:3]}, model {cm['depth'][bad][:3]}, bound {derr[bad][:3]})")
            # where the model's v = z (2^24 - 1) is farther from k + 1/2 than v's bound (ez (2^24 - 1) and the roundings of the product
            # and of the + 0.5, u (v + 1) each), rounding to nearest gives ONE depth: the twin's must be the model's
            with np.errstate(all="ignore"):
                v = z.v * D
                decided = both & (np.abs(v - np.floor(v) - 0.5) > z.e * D + 2 * U * (np.abs(v) + 1)) & np.isfinite(z.e)
            bad = decided & (ct["depth"] != cm["depth"])
            if bad.any():
                problems.append(f"tri {tri}.{sub}: depth is not the nearest step at {int(bad.sum())} pixels where rounding is decided "
                                f"(twin {ct['depth'][bad][:3]}, z (2^24 - 1) = {v[bad][:3]})")
            n_decided[0] += int((decided & (v - np.floor(v) > 0.5)).sum())
            n_decided[1] += int((decided & (v - np.floor(v) < 0.5)).sum())
            either = ct["inside"] | cm["inside"]
            px_exempt[ct["yy"][either & fex], ct["xx"][either & fex]] = True
            if bulk[tri]:
                n_frag += int(either.sum())
                n_ex += int((either & fex).sum())
            frag_store.append((pm, cm, derr))
            evs[(tri, sub)] = (s, tu, tv)
    # ---- per pixel: the model's winner against its runner-up
    index_of = {id(p): i for i, p in enumerate(M["pieces"])}
    for pm, cm, derr in frag_store:
        won = cm["inside"] & (M["piece_index"][cm["yy"], cm["xx"]] == index_of[id(pm)])
        derr_win[cm["yy"][won], cm["xx"][won]] = derr[won]
    tie = np.zeros((H, W), bool)
    for pm, cm, derr in frag_store:
        ins = cm["inside"]
        lost = ins & (M["piece_index"][cm["yy"], cm["xx"]] != index_of[id(pm)])
        close = lost & (cm["depth"] - derr <= M["depth"][cm["yy"], cm["xx"]] + derr_win[cm["yy"], cm["xx"]])
        tie[cm["yy"][close], cm["xx"][close]] = True
    ok = ~px_exempt & ~tie
    bad = ok & ((T["tri"] != M["tri"]) | (T["piece"] != M["piece"]))
    if bad.any():
        yy, xx = np.nonzero(bad)
        problems.append(f"winner differs at {int(bad.sum())} pixels, first ({xx[0]}, {yy[0]}): twin tri {T['tri'][yy[0], xx[0]]} "
                        f"model tri {M['tri'][yy[0], xx[0]]}")
    same = ok & T["covered"] & M["covered"] & (T["tri"] == M["tri"]) & (T["piece"] == M["piece"])
    bad = same & (np.abs(T["depth"] - M["depth"]) > derr_win)
    if bad.any():
        problems.append(f"winning depth beyond its bound at {int(bad.sum())} pixels")
    # ---- grey of the common winner
    lips = level_lipschitz(levels)
    tw, th = float(levels[0].shape[1]), float(levels[0].shape[0])
    gmax = 0.0
    for (tri, sub), (s, tu, tv) in evs.items():
        sel = same & (T["tri"] == tri) & (T["piece"] == sub)
        if not sel.any():
            continue
        yy, xx = np.nonzero(sel)
        pt = tw_pieces[(tri, sub)]
        u, v, rho2, lam = shade_ev(s, tu, tv, pt["t"]["x_lo"], pt["t"]["y_lo"], xx.astype(np.float64), yy.astype(np.float64), tw, th)
        for name, ev in (("u", u), ("v", v), ("rho2", rho2)):
            got = T[name][yy, xx].astype(np.float64)
            with np.errstate(all="ignore"):
                bad = ~(np.abs(got - ev.v) <= ev.e) & np.isfinite(ev.e) & np.isfinite(got)
            if bad.any():
                bound_problems.append(f"tri {tri}.{sub}: {name} off by more than its bound at {int(bad.sum())} pixels "
                                      f"({np.abs(got - ev.v)[bad].max():.3g} > {ev.e[bad].min():.3g})")
        with np.errstate(all="ignore"):
            mini = (rho2.v - rho2.e > 1) & np.isfinite(lam.e)
            bad = mini & ~(np.abs(T["lam"][yy, xx].astype(np.float64) - lam.v) <= lam.e)
        if bad.any():
            bound_problems.append(f"tri {tri}.{sub}: lambda off by more than its bound at {int(bad.sum())} pixels")
        G = grey_bound(levels, lips, u, v, rho2, lam)
        dg = np.abs(T["grey"][yy, xx].astype(np.int64) - M["grey"][yy, xx].astype(np.int64))
        with np.errstate(all="ignore"):
            dl = np.abs(np.clip(T["luma"][yy, xx].astype(np.float64), 0, 1) - np.clip(M["luma"][yy, xx], 0, 1)) * 255
            fin = np.isfinite(dl)
        if (dl[fin] > G[fin]).any():
            k = int(np.argmax(np.where(fin, dl - G, -np.inf)))
            problems.append(f"tri {tri}.{sub}: luma x 255 differs by {dl[k]:.4g} > bound {G[k]:.4g} at ({xx[k]}, {yy[k]})")
        if (dg > G + 1).any():
            problems.append(f"tri {tri}.{sub}: grey differs by more than its bound + 1 at {int((dg > G + 1).sum())} pixels")
        gmax = max(gmax, float(G.max()))
        if bulk[tri]:
            n_grey, n_loose = n_grey + len(G), n_loose + int((G >= 1.0).sum())
    return {"problems": problems, "bound_problems": bound_problems, "frags": n_frag, "frags_exempt": n_ex,
            "pixels": int((T["covered"] | M["covered"]).sum()), "pixels_exempt": int(((T["covered"] | M["covered"]) & ~ok).sum()),
            "grey_bound_max": gmax, "grey_pixels": n_grey, "grey_loose": n_loose, "depth_decided_up": n_decided[0],
            "depth_decided_down": n_decided[1], "twin": T, "model": M}
