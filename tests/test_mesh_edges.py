"""Edges of the textured-mesh renderer: the fp32 twin (oracle/mesh_oracle_np.py, render_staged) against the float64 model of the same
rule (render_mesh_f64) on hard meshes, textures and views (tests/helpers/mesh_cases.py); then (GPU) every mesh path of the product
against the twin on every family, at frame sizes with and without whole dwords and tiles.

The float64 criterion (tests/helpers/mesh_bounds.py).  Every bound is the standard model of fp32 rounding, fl(a o b) = (a o b)(1 + d),
|d| <= u = 2^-24, carried through the twin's own sequence of operations (Ev: a float64 value with a bound on how far the fp32 value
may be from it; the rules for +, -, *, / and max are in that module's docstring).  Per (triangle, view):
    clip coordinates  |c_r(fp32) - c_r| <= E_r = 3u T_r, T_r = sum_j |m_rj p_j| + |m_r3|       (the point renderer's bound);
    d = cz + cw       within E_z + E_w + u |d|: which corners the near plane cuts off, and the cut t = d_i / (d_i - d_o) with the
                      corners interpolated from it;
    window            rho = c / cw within (E_r + |rho| E_w) / (cw - E_w) + u |rho|, then xw = (rho / 2 + 1/2) W, yw, zw and 1 / cw;
    area, edge values area = (x1 - x0)(y2 - y0) - (x2 - x0)(y1 - y0) and b_k = (ex_k (py - y_a) - ey_k (px - x_a)) / area from the
                      window bounds: B_k, the bound on b_k, is what decides coverage;
    z, depth          z = sum b_k zw_k within its bound ez; round(z (2^24 - 1)) in fp32 rounds the product and the + 0.5 at a spacing
                      of at most 1, so the depths differ by at most ceil(ez (2^24 - 1) + 2) steps;
    u, v, lambda      the three attribute planes, the three reciprocals, rho2 and lambda = log2(rho2) / 2 with
                      d lambda <= d rho2 / (2 ln 2 (rho2 - d rho2)) + 4u |lambda| + 2^-22 (log2f within 2 ulp);
    grey              the sampled luma is continuous in (u, v, lambda) with Lipschitz constants given by the levels' largest
                      neighbouring-texel differences and by |s_(l+1) - s_l| at this uv (grey_bound's docstring), so
                      |luma(fp32) - luma| 255 <= G, and the rounded greys differ by at most G + 1.
A fragment is EXEMPT when a float64 quantity lies within its bound of a decision: a corner's d of 0 (which corners are clipped: the
whole triangle), cw of 0, a clip test (no corner inside a plane by more than its bound while not all are outside by more), the
area of 0, a box bound of its rounding decision (set-up: the whole piece); |b_k| <= B_k (coverage), z within ez of 0 or 1, or a bound
that is not finite (fp32 overflow, a subnormal divisor).  A pixel is exempt from the winner check when one of its fragments is
exempt or when the model's winner and another fragment are closer than the sum of their depth bounds.  Elsewhere: the same corners
clipped, the same set-up decision and box, the same coverage, the same winner, depths within their bound, grey within G + 1.
Where the grey criterion cannot see: G grows with |u| du (|u| ~ 500: du ~ 1e-4, a twentieth of a texel on a 100-texel side of noise),
with 1 / (rho2 - d rho2) (footprints near 0: tiny boxes, constant uv) and is 255 where a bound is not finite (the matrix x 2^-130,
grazing planes' horizon).  On those pixels only GPU == twin says anything about the grey; test_twin_meets_float64_model_per_pixel
prints, per family, on how many compared pixels G is a whole grey level or more.
Triangles built ON a decision boundary (a case's bulk mask is False) are exempt by construction; of every family's other
fragments at most BULK_EXEMPT may be exempt -- the point renderer's cap -- so that the exemption cannot swallow a family.
far_from_origin at 1,000 m is the one exception (nobody has measured how far from the origin fp32 holds): the criterion and the
bounds are asserted there, the exempt share is printed (profiles/NOTES.md has the figures).

GPU against the twin.  Coverage, winner and depth decisions are the same fp32 operations on both sides, and so is all of the
shading but log2f: pixels the twin magnifies (rho2 <= 1: no logarithm) must be byte-equal.  A minified pixel may differ, by 1,
only where the rounding of its grey can turn on the logarithm's last bit: with each side's log2f within 1 ulp of log2(rho2) = L,
the two lambdas = L / 2 differ by at most 2 ulp(L) / 2 <= 2^-23 |L| = 2^-22 |lambda|; f = lambda - floor(lambda) carries that
difference (exactly: the subtraction is exact), luma = s0 + (s1 - s0) f changes by |s1 - s0| 2^-22 lambda plus four roundings
of values below 1 (two per side), v = clip(luma) 255 by 255 times that plus one rounding per side:
    eps = 255 (|s1 - s0| 2^-22 lambda + 6u),
with |s1 - s0| replaced by 1 where f is within 2^-22 lambda of 0 or 1 (the two sides may blend different level pairs there; luma is
continuous across it and no two samples differ by more than 1).  The twin's grey may differ from the device's only where
|v - floor(v) - 0.5| <= eps.
"""
import functools
import time

import numpy as np
import pytest

from helpers import mesh_bounds as mb
from helpers import mesh_cases as mc
from helpers import render_cases as rc
from oracle import mesh_oracle_np as mo

try:
    import torch
except ImportError:  # the CPU tier does not need it
    torch = None

f32 = np.float32
U = 2.0 ** -24
CPU_SIZES = [(64, 48), (320, 240), (150, 90)]
BULK_EXEMPT = 0.02            # the point renderer's cap (test_render_edges.py)
ALL_ON_BOUNDARIES = {"pixel_centres", "huge_uv"}      # families without bulk triangles
FAMILIES = list(mc.EXPECTED_BRANCHES)
# Families whose criterion is a Python loop over thousands of triangles or millions of fragments: per fragment at ONE size (the
# per-pixel test's), not three.  Their branches are still checked at all three sizes, their kernels at all four GPU sizes.
HEAVY = {"full_bins", "frustum_margin", "far_from_origin", "tessellation", "depth"}


SLOW_REACH = {"full_bins", "frustum_margin", "far_from_origin"}


def cpu_sizes(family):
    return [(150, 90)] if family in HEAVY else CPU_SIZES


@functools.lru_cache(maxsize=None)
def levels_of(family, W, H, i):
    return mo.mip_luma(mc.family(family, W, H)[i]["rgb"])


@functools.lru_cache(maxsize=None)
def analysed(family, W, H):
    """compare_view for every (case, view) of a family (the staged renders dropped: they are large)."""
    out = []
    for i, c in enumerate(mc.family(family, W, H)):
        if not c.get("criterion", True):        # (full_bins: the bin counts are the kernels' business)
            continue
        S = len(c["mvps"])
        views = range(S) if S <= 4 else sorted({0, S // 2, S - 1})
        if "distance" in c:
            views = (3,)          # (far_from_origin: three distances of the tessellation, whose own family takes all four views)
        for s in views:      # (many-view cases: the first, middle and last views)
            r = mb.compare_view(c["xyz"], c["uv"], levels_of(family, W, H, i), c["mvps"][s], W, H, c["bulk"])
            r.pop("twin"), r.pop("model")
            r.update(case=i, view=s, distance=c.get("distance"))
            out.append(r)
    return out


# ----------------------------------------------------------------------------------------------------- CPU tier
@pytest.mark.parametrize("shape", CPU_SIZES, ids=[f"{w}x{h}" for w, h in CPU_SIZES])
def test_families_reach_their_branches(shape):
    W, H = shape
    fams = mc.families(W, H)
    assert set(fams) == set(mc.EXPECTED_BRANCHES)
    for fam, lst in fams.items():
        if fam in SLOW_REACH and shape != (150, 90):
            continue          # (thousands of triangles whose branches do not depend on the frame: one size)
        seen = mc.reached(lst, W, H)
        missing = mc.EXPECTED_BRANCHES[fam] - seen
        assert not missing, f"{W}x{H} {fam}: does not reach {missing}"
        assert all(len(c["xyz"]) // 3 <= 400 for c in lst), fam
        print(f"{W}x{H} {fam}: {sorted(seen)}")


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("shape", CPU_SIZES, ids=[f"{w}x{h}" for w, h in CPU_SIZES])
def test_twin_meets_float64_model_per_fragment(family, shape):
    """Same corners clipped, same set-up, same coverage, depth within its bound, for every fragment outside the exemption; and the
    exemption holds at most BULK_EXEMPT of the family's bulk fragments."""
    W, H = shape
    if shape not in cpu_sizes(family):
        return      # (HEAVY: one size)
    res = analysed(family, W, H)
    per_pixel = ("winner", "winning", "luma", "grey")        # (the next test's)
    bad = [f"[{r['case']}] view {r['view']}: {p}" for r in res for p in r["problems"] if not any(k in p for k in per_pixel)]
    assert not bad, bad[:8]
    for dist in sorted({r["distance"] for r in res}, key=lambda d: -1 if d is None else d):
        sel = [r for r in res if r["distance"] == dist]
        n, n_ex = sum(r["frags"] for r in sel), sum(r["frags_exempt"] for r in sel)
        print(f"{family} {W}x{H}" + (f" at {dist:g} m" if dist is not None else "") + f": {n_ex} of {n} bulk fragments exempt"
              + (f" ({n_ex / n:.2e})" if n else ""))
        if dist is not None and dist >= 1000.0:
            continue
        assert (n == 0) == (family in ALL_ON_BOUNDARIES), (family, n)
        assert n_ex <= BULK_EXEMPT * n, f"{family}: {n_ex} of {n} fragments off the boundaries exempt"


@pytest.mark.parametrize("family", FAMILIES)
def test_twin_meets_float64_model_per_pixel(family):
    """Outside the exemption every pixel has the model's winner, its depth within the bound, and its grey within G + 1."""
    W, H = 150, 90
    res = analysed(family, W, H)
    bad = [f"[{r['case']}] view {r['view']}: {p}" for r in res for p in r["problems"]]
    assert not bad, bad[:8]
    n, n_ex = sum(r["pixels"] for r in res), sum(r["pixels_exempt"] for r in res)
    print(f"{family}: {n_ex} of {n} covered pixels exempt from the winner check; largest grey bound {max(r['grey_bound_max'] for r in res):.3g}")
    g, loose = sum(r["grey_pixels"] for r in res), sum(r["grey_loose"] for r in res)
    print(f"{family}: grey compared on {g} bulk pixels, the bound is a whole grey level or more on {loose}" + (f" ({loose / g:.1%})" if g else ""))


def test_bound_holds():
    """Every derived bound holds against the twin on every family: clip coordinates within E_r, window coordinates, 1 / cw, area, the
    edge values, z, u, v, rho2 and lambda within their Ev bounds (depth and grey: the two tests above)."""
    for fam in FAMILIES:
        for W, H in cpu_sizes(fam):
            bad = [f"{W}x{H} {fam}[{r['case']}] view {r['view']}: {p}" for r in analysed(fam, W, H) for p in r["bound_problems"]]
            assert not bad, bad[:8]


def test_exemption_is_rare_on_an_ordinary_mesh():
    from test_render import ground_mesh, plane_mesh
    W, H = 160, 120
    m = rc.cameras(W, H)["oblique"]
    n = n_ex = 0
    for xyz, uv, rgb, _ in (plane_mesh(W, H), ground_mesh(W, H)):
        r = mb.compare_view(xyz.astype(f32), uv.astype(f32), mo.mip_luma(rgb), m, W, H)
        assert not r["problems"] and not r["bound_problems"], (r["problems"][:5], r["bound_problems"][:5])
        n, n_ex = n + r["frags"], n_ex + r["frags_exempt"]
    assert n > 5000 and n_ex < 0.005 * n, (n_ex, n)


def _inside_outline(outline, m, W, H, margin=1e-3):
    """Pixels whose centres lie inside the projected quadrilateral `outline` (world corners) by more than margin pixels, in float64."""
    M = np.asarray(m, f32).astype(np.float64).reshape(4, 4).T
    c = np.c_[outline, np.ones(4)] @ M.T
    q = np.c_[(c[:, 0] / c[:, 3] * 0.5 + 0.5) * W, (c[:, 1] / c[:, 3] * 0.5 + 0.5) * H]
    if (q[1, 0] - q[0, 0]) * (q[2, 1] - q[0, 1]) - (q[2, 0] - q[0, 0]) * (q[1, 1] - q[0, 1]) < 0:
        q = q[::-1]
    yy, xx = np.mgrid[0:H, 0:W]
    px, py = xx + 0.5, yy + 0.5
    inside = np.ones((H, W), bool)
    for k in range(4):
        a, b = q[k], q[(k + 1) % 4]
        e = b - a
        inside &= (e[0] * (py - a[1]) - e[1] * (px - a[0])) / np.hypot(*e) > margin
    return inside


@pytest.mark.parametrize("shape", CPU_SIZES, ids=[f"{w}x{h}" for w, h in CPU_SIZES])
def test_tessellation_has_no_cracks(shape):
    """Every pixel inside the projected outline of a closed mesh is covered, in the twin and in the model: shared edges leave no
    gap (and, by the top-left rule, no pixel twice: nfrag is 1 there)."""
    W, H = shape
    for fam in ("tessellation", "far_from_origin") if shape == (150, 90) else ("tessellation",):
        for c in mc.family(fam, W, H):
            lv = mo.mip_luma(c["rgb"])
            outline = c["outline"] if "outline" in c else None
            for s, m in enumerate(c["mvps"]):
                if outline is None:      # far_from_origin: the tessellation's outline, moved along
                    base = mc.family("tessellation", W, H)[0]
                    inside = _inside_outline(base["outline"], base["mvps"][s], W, H, margin=0.05 if c["distance"] else 1e-3)
                else:
                    inside = _inside_outline(outline, m, W, H)
                assert inside.mean() > 0.2
                for name, st in (("twin", mo.render_staged(c["xyz"], c["uv"], lv, m, W, H)), ("model", mo.render_mesh_f64(c["xyz"], c["uv"], lv, m, W, H))):
                    assert st["covered"][inside].all(), f"{fam} {c['note']} view {s}: {(~st['covered'] & inside).sum()} uncovered pixels in the {name}"
                    assert (st["nfrag"][inside] == 1).all(), f"{fam} {c['note']} view {s}: a pixel drawn twice in the {name}"


def _top_left_owner(window_tris, W, H):
    """The triangle that owns each pixel by the top-left rule, stated without edge functions: a sample exactly on an edge belongs
    to the triangle whose interior holds the sample moved a little to the right and much less than that down (a left edge has the
    interior on its right; a horizontal top edge has it below; right and bottom edges lose).  Exact half-integer corners, float64."""
    yy, xx = np.mgrid[0:H, 0:W]
    px, py = xx + 0.5 + 1e-3, yy + 0.5 - 1e-6
    owner = np.full((H, W), -1)
    count = np.zeros((H, W), int)
    for i, t in enumerate(window_tris):
        ins = np.ones((H, W), bool)
        for k in range(3):
            a, b = t[k], t[(k + 1) % 3]
            ins &= (b[0] - a[0]) * (py - a[1]) - (b[1] - a[1]) * (px - a[0]) > 0
        owner[ins] = i
        count += ins
    assert count.max() == 1
    return owner


@pytest.mark.parametrize("shape", [(64, 32), (64, 48), (150, 90), (320, 240)], ids=["64x32", "64x48", "150x90", "320x240"])
def test_pixel_centres_have_exactly_one_owner(shape):
    """Edges through pixel centres with exact fp32 window coordinates: every pixel on a shared edge, and the fan's common vertex,
    gets exactly one fragment, and it is the top-left owner's.  On 64 x 32 (powers of two) the float64 model sees the same
    coordinates and must agree."""
    W, H = shape
    for c in mc.family("pixel_centres", W, H):
        lv = mo.mip_luma(c["rgb"])
        owner = _top_left_owner(c["window"], W, H)
        on_edges = 0
        for name, st in (("twin", mo.render_staged(c["xyz"], c["uv"], lv, EXACT, W, H, keep_cover=True)),
                         ("model", mo.render_mesh_f64(c["xyz"], c["uv"], lv, EXACT, W, H, keep_cover=True))):
            if name == "model" and (W & (W - 1) or H & (H - 1)):
                continue
            for p in st["pieces"]:
                assert p["t"]["status"] == "kept"
                assert (np.array([p["t"]["xw"], p["t"]["yw"]]).T == np.array(c["window"][p["tri"]])).all(), "window coordinates are not exact"
                on_edges += sum(int((b == 0).sum()) for b in p["cover"]["b"])
            assert (st["nfrag"] == (owner >= 0)).all(), f"{c['note']} ({name}): {(st['nfrag'] != (owner >= 0)).sum()} pixels with another fragment count"
            assert (st["tri"] == owner).all(), f"{c['note']} ({name}): {(st['tri'] != owner).sum()} pixels with another owner"
            greys = {int(g) for g in st["grey"][owner >= 0]}
            assert len(greys) == len(c["window"]), "the triangles' greys do not tell them apart"
        assert on_edges > 10


EXACT = mc.EXACT
WRAP_SIDES = (1, 2, 3, 5, 6, 7, 12, 25, 50, 100, 127, 640, 1000, 3000, 32767, 32768)
WRAP_REACH = (2.0 ** 20, 2.0 ** 24, 2.0 ** 26, 2.0 ** 31, 1e12, 1e30, float(np.finfo(f32).max))


def _wrap_inputs(reach, n, rng):
    """Integer-valued fp32 x up to +-reach: random, and the ends of the domain around 2^24 - n."""
    x = np.floor(rng.uniform(-1, 1, 20000) * reach).astype(f32)
    edge = np.arange(-3, 4, dtype=np.float64)
    special = np.concatenate([edge, 2.0 ** 24 - n + edge, -(2.0 ** 24 - n) + edge, np.array([reach, -reach]), n * np.arange(-3, 4.0),
                              n * np.floor(reach / n) + edge])
    return np.concatenate([x, special[np.abs(special) <= reach].astype(f32)])


def test_wrap_index_stays_in_range():
    """wrap_index (the fp32 restatement of the kernel's) gives an index in [0, n) for every float, and x mod n inside its domain
    |x| < 2^24 - n; the rule before the bound (bounded=False) leaves [0, n) -- by gigabytes in the end -- so this test sees it."""
    rng = np.random.default_rng(0)
    old_out_of_range = {}
    for n in WRAP_SIDES:
        for reach in WRAP_REACH:
            x = _wrap_inputs(reach, n, rng)
            got = mo.wrap_index(x, n)
            assert ((got >= 0) & (got < n)).all(), (n, reach, x[(got < 0) | (got >= n)][:5])
            dom = np.abs(x.astype(np.float64)) < 2.0 ** 24 - n
            assert (got[dom] == np.mod(x[dom].astype(np.int64), n)).all(), (n, reach)
            old = mo.wrap_index(x, n, bounded=False)
            assert (old[dom] == got[dom]).all(), (n, reach)         # inside the domain the bound changes nothing
            off = np.maximum(old - (n - 1), -old).max()
            if off > 0:
                old_out_of_range[n] = max(old_out_of_range.get(n, 0), int(off))
        special = np.array([np.inf, -np.inf, np.nan, 0.0, -0.0], f32)
        got = mo.wrap_index(special, n)
        assert ((got >= 0) & (got < n)).all() and (got == 0).all(), (n, got)
    print("the unbounded rule's largest excursion beyond [0, n), by n:", old_out_of_range)
    # the rule of the parent commit fails this test: out of range for every side that is not a power of two (n = 1: x - x = 0 always)
    assert set(old_out_of_range) >= {n for n in WRAP_SIDES if n & (n - 1)}, old_out_of_range
    assert not any(n & (n - 1) == 0 and n < 32768 for n in old_out_of_range), old_out_of_range
    assert old_out_of_range[3] >= 2 ** 31 - 1 and old_out_of_range[7] > 60000       # (int) of 7.6e22 saturates; tens of thousands at 1e12


def test_twin_nonfinite_rules():
    """The device's conversions, stated: float -> int saturates and NaN converts to 0; fminf(fmaxf(NaN, 0), 1) is 0 (grey 0); a NaN
    rho2 takes the magnification branch; a triangle with a NaN or inf corner draws nothing and changes no neighbour."""
    big = np.array([np.nan, np.inf, -np.inf, 3e9, -3e9, 1e30, -7.9, 7.9], f32)
    assert list(mo.sat_int(big)) == [0, 2 ** 31 - 1, -2 ** 31, 2 ** 31 - 1, -2 ** 31, 2 ** 31 - 1, -7, 7]
    assert list(mo.sat_uint(big)) == [0, 2 ** 32 - 1, 0, 3000000000, 0, 2 ** 32 - 1, 0, 7]
    W, H = 64, 48
    c = mc.family("nonfinite", W, H)[0]
    lv = mo.mip_luma(c["rgb"])
    T = len(c["xyz"]) // 3
    with np.errstate(all="ignore"):
        bad_tri = ~np.isfinite(c["xyz"].reshape(T, 9)).all(1)
        bad_uv = ~np.isfinite(c["uv"].reshape(T, 6)).all(1)
    assert bad_tri.sum() >= 6 and bad_uv.sum() >= 3
    for m in c["mvps"]:
        st = mo.render_staged(c["xyz"], c["uv"], lv, m, W, H)
        assert not np.isin(st["tri"], np.flatnonzero(bad_tri)).any()
        keep = np.repeat(~bad_tri, 3)
        alone = mo.render_staged(c["xyz"][keep], c["uv"][keep], lv, m, W, H)
        assert (alone["grey"] == st["grey"]).all()
        won = np.isin(st["tri"], np.flatnonzero(bad_uv))
        if won.any():
            assert (st["grey"][won] == 0).all() and np.isnan(st["luma"][won]).all()
    # an infinite uv at one corner: u and the differences ux - u are inf - inf; rho2 is NaN: the base level, no logarithm, grey 0
    t = mo.setup(W, H, *(np.array(v, f32) for v in ([-0.5, 0.5, -0.5], [-0.5, -0.5, 0.5], [0, 0, 0], [1, 1, 1])))
    assert t["status"] == "kept"
    sh = mo.shade(t, np.array([0.1, np.inf, 0.1], f32), np.array([0.2, 0.2, 0.9], f32), lv, np.array([20]), np.array([15]))
    assert np.isnan(sh["rho2"]).all() and (sh["l0"] == 0).all() and (sh["l1"] == 0).all() and (sh["grey"] == 0).all()


def test_depth_rounds_to_nearest():
    """The depth is round(z (2^24 - 1)), not its truncation.  The general depth bound (2 steps and more) cannot tell the two apart;
    next to the near plane under the EXACT matrix it can be decided: z (2^24 - 1) is a few tens of thousands, known to a few
    hundredths of a step (compare_view: `decided`), and there the twin's depth must equal the model's -- for fragments that round
    up as for those that round down."""
    res = analysed("depth", 150, 90)
    assert not [p for r in res for p in r["problems"] if "nearest" in p]
    last = [r for r in res if r["case"] == max(x["case"] for x in res)][0]
    assert last["depth_decided_up"] > 500 and last["depth_decided_down"] > 500, (last["depth_decided_up"], last["depth_decided_down"])


def test_twin_attribute_rounding_is_pinned():
    """A change detector, not a criterion: a digest of the twin's per-pixel winner and uv BITS on two ordinary meshes.  Everything
    up to the logarithm is IEEE fp32 arithmetic in a fixed order, the same on every machine.  The float64 criterion bounds the
    twin's error and so cannot see a reordering that stays inside the bounds -- the attribute planes taken about the corner of
    the box's first pixel instead of its centre are the same planes, rounded differently, exact wherever uv is exactly
    representable -- but the kernels are held to the twin byte for byte, so the twin's rounding order is part of what the GPU tier
    checks.  The digest was taken from this twin when the MI355X kernels equalled it on every pixel of the GPU tier; it changes
    only together with the kernels' arithmetic."""
    import hashlib
    from test_render import _both_windings, ground_mesh, plane_mesh
    W, H = 96, 72
    h = hashlib.sha256()
    for xyz, uv, rgb, _ in (plane_mesh(W, H), ground_mesh(W, H)):
        xyz, uv = _both_windings(xyz, uv)
        for cam in ("axis", "oblique"):
            st = mo.render_staged(xyz, uv, mo.mip_luma(rgb), rc.cameras(W, H)[cam], W, H)
            assert st["covered"].mean() > 0.3
            for k in ("tri", "piece"):
                h.update(np.ascontiguousarray(st[k], np.int64).tobytes())
            for k in ("u", "v"):
                h.update(np.ascontiguousarray(st[k], np.float32).view(np.uint32).tobytes())
    assert h.hexdigest() == "eba280b6778616b7f9d40508cbfdca9dd32be566877b1c4e7e8eb7085e380838", h.hexdigest()


@pytest.mark.parametrize("side", list(mc.TEXTURE_SIDES) + [(37, 1), (5, 2)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_mip_chain_odd_sides(side):
    """mip_luma's level shapes and values for sides that are not powers of two, against a direct float64 2x2 box: level l + 1 has
    max(1, floor(side / 2)) texels a side, texel (i, j) the rounded mean of texels (min(2i, w - 1), min(2i + 1, w - 1)) x (rows
    likewise) of level l's RGB8 (the last column / row of an odd side is dropped; a side of 1 repeats its texel)."""
    w, h = side
    rgb = mc.noise_texture(w, h, 5, 0, 255)
    lv = mo.mip_luma(rgb)
    cur = rgb.astype(np.float64)
    shapes = []
    l = 0
    while True:
        ch, cw = cur.shape[:2]
        shapes.append((ch, cw))
        exp = (0.299 * cur[..., 0] + 0.587 * cur[..., 1] + 0.114 * cur[..., 2]) / 255
        assert lv[l].shape == (ch, cw) and np.abs(lv[l] - exp).max() <= 4 * U, (l, np.abs(lv[l] - exp).max())
        if cw == 1 and ch == 1:
            break
        nw, nh = max(1, cw // 2), max(1, ch // 2)
        nxt = np.zeros((nh, nw, 3))
        for j in range(nh):
            for i in range(nw):
                xs, ys = [min(2 * i, cw - 1), min(2 * i + 1, cw - 1)], [min(2 * j, ch - 1), min(2 * j + 1, ch - 1)]
                nxt[j, i] = np.floor(sum(cur[y, x] for y in ys for x in xs) / 4 + 0.5)
        cur, l = nxt, l + 1
    assert len(lv) == len(shapes)


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


def twin_stack(c, W, H, mvps=None, xyz=None, uv=None):
    lv = mo.mip_luma(c["rgb"])
    mvps = c["mvps"] if mvps is None else mvps
    return [mo.render_staged(c["xyz"] if xyz is None else xyz, c["uv"] if uv is None else uv, lv, m, W, H) for m in mvps]


DIFFERING = {}     # family -> [pixels that differ from the twin, minified pixels, covered pixels], for the record (printed)


def against_twin(tag, got, staged, family=None):
    """The GPU-vs-twin criterion of the module docstring for a render stack -> list of complaints."""
    bad = []
    for s, st in enumerate(staged):
        g, e = got[s].astype(np.int64), st["grey"].astype(np.int64)
        diff = g != e
        cov = st["covered"]
        with np.errstate(all="ignore"):
            mini = cov & (st["rho2"] > 1)
            lam = np.where(mini, st["lam"].astype(np.float64), 0.0)
            dl = 2.0 ** -22 * lam
            f = st["f"].astype(np.float64)
            ds = np.where((f < dl) | (1 - f < dl), 1.0, np.abs(st["s1"].astype(np.float64) - st["s0"].astype(np.float64)))
            eps = 255 * (ds * dl + 6 * U)
            v = np.clip(st["luma"].astype(np.float64), 0, 1) * 255
            may = mini & (np.abs(v - np.floor(v) - 0.5) <= eps) & (np.abs(g - e) <= 1)
        if family is not None:
            rec = DIFFERING.setdefault(family, [0, 0, 0])
            rec[0], rec[1], rec[2] = rec[0] + int(diff.sum()), rec[1] + int(mini.sum()), rec[2] + int(cov.sum())
        wrong = diff & ~may
        if wrong.any():
            yy, xx = np.nonzero(wrong)
            bad.append(f"{tag} view {s}: {int(wrong.sum())} px differ outside the criterion ({int((wrong & ~mini).sum())} not minified), first ({xx[0]}, {yy[0]}): "
                       f"got {g[yy[0], xx[0]]} twin {e[yy[0], xx[0]]} v {v[yy[0], xx[0]]:.6f} eps {eps[yy[0], xx[0]]:.2e}")
    return bad


def masks_differ(tag, got, staged):
    return [f"{tag} view {s}: {(got[s] != st['covered']).sum()} px" for s, st in enumerate(staged) if not (got[s] == st["covered"].astype(np.uint8)).all()]


# 160 x 120: whole dwords; 150 x 90: width % 4 != 0 (the byte-store tail); 40 x 30: smaller than a tile; 130 x 129: a 2-pixel last
# tile column and a 1-pixel last tile row
GPU_SIZES = [(160, 120), (150, 90), (40, 30), (130, 129)]
NOT_BEFORE_THE_FIX = {"huge_uv"}     # test_gpu_huge_uv_is_safe's: never sent to a library whose wrap_index is not bounded


@pytest.mark.gpu
@pytest.mark.parametrize("family", [f for f in FAMILIES if f not in NOT_BEFORE_THE_FIX])
@pytest.mark.parametrize("shape", GPU_SIZES, ids=[f"{w}x{h}" for w, h in GPU_SIZES])
def test_gpu_render_mesh_families(nmi, family, shape):
    """nmi_render_mesh and nmi_render_mesh_masked against the twin (the criterion above; the masks equal the twin's coverage), one
    image whatever the tile queue's and the clip queue's capacity, and the same mesh after nmi_sort_triangles against the twin of
    the SORTED arrays (draw order decides ties)."""
    W, H = shape
    bad = []
    t0 = time.time()
    with nmi.NmiContext(W, H) as ctx:
        for i, c in enumerate(mc.family(family, W, H)):
            tag = f"{family}[{i}]"
            staged = twin_stack(c, W, H)
            dx, du = dev(c["xyz"]), dev(c["uv"])
            with nmi.NmiTexture(ctx, c["rgb"]) as tex:
                got = ctx.render_mesh(dx, du, tex, c["mvps"]).cpu().numpy()
                bad += against_twin(tag + " render", got, staged, family)
                r2, m2 = ctx.render_mesh_masked(dx, du, tex, c["mvps"])
                if not (r2.cpu().numpy() == got).all():
                    bad.append(f"{tag}: the masked render differs from the plain one")
                bad += masks_differ(tag + " mask", m2.cpu().numpy(), staged)
                for cap, clip_cap in ((5, 1 << 18), (0, 1 << 18), (4 << 20, 2)):
                    ctx.set_option(ctx.OPT_TILE_QUEUE, cap)
                    ctx.set_option(ctx.OPT_CLIP_QUEUE, clip_cap)
                    if not (ctx.render_mesh(dx, du, tex, c["mvps"]).cpu().numpy() == got).all():
                        bad.append(f"{tag}: tile queue {cap} / clip queue {clip_cap} gives another image")
                ctx.set_option(ctx.OPT_TILE_QUEUE, 4 << 20)
                ctx.set_option(ctx.OPT_CLIP_QUEUE, 1 << 18)
                sx, su = ctx.sort_triangles(dx, du)
                sorted_twin = twin_stack(c, W, H, xyz=sx.cpu().numpy(), uv=su.cpu().numpy())
                bad += against_twin(tag + " sorted", ctx.render_mesh(sx, su, tex, c["mvps"]).cpu().numpy(), sorted_twin)
    print(f"{family} {W}x{H}: {DIFFERING.get(family)} [differing, minified, covered] pixels so far; {time.time() - t0:.1f} s")
    assert not bad, bad[:10]


def _replays(c):
    """A level's parameters replay after replay: the case's views, every view moved by a small world translation, the case's
    views again (whatever the second replay binned or queued must not linger)."""
    m2 = rc.shifted(c["mvps"], (0.07, -0.05, 0.3))
    assert all(not np.array_equal(a, b) for a, b in zip(c["mvps"], m2)), "a replay's view did not change"
    return [c["mvps"], m2, c["mvps"]]


@pytest.mark.gpu
@pytest.mark.parametrize("family", [f for f in FAMILIES if f not in NOT_BEFORE_THE_FIX])
@pytest.mark.parametrize("shape", GPU_SIZES, ids=[f"{w}x{h}" for w, h in GPU_SIZES])
def test_gpu_mesh_level_families(nmi, family, shape):
    """A mesh NmiLevel, plain and covered, over three replays with changing matrices: renders and coverage against the twin."""
    W, H = shape
    bad = []
    with nmi.NmiContext(W, H) as ctx:
        frame = dev(np.random.default_rng(0).integers(0, 256, (H, W), dtype=np.uint8))
        for i, c in enumerate(mc.family(family, W, H)):
            dx, du = dev(c["xyz"]), dev(c["uv"])
            S = len(c["mvps"])
            replays = _replays(c)
            twins = [twin_stack(c, W, H, mv) for mv in replays[:2]]
            twins.append(twins[0])
            with nmi.NmiTexture(ctx, c["rgb"]) as tex:
                for covered in (False, True):
                    with nmi.NmiLevel(ctx, dx, du, frame, S, 1, 1.0, texture=tex) as lv:
                        if covered:
                            lv.set_coverage(True)
                        for rep, mv in enumerate(replays):
                            lv.run(mv, np.eye(3)[None])
                            tag = f"{family}[{i}] {'covered ' if covered else ''}level replay {rep}"
                            bad += against_twin(tag, lv.outputs()[0], twins[rep])
                            if covered:
                                bad += masks_differ(tag + " coverage", lv.coverage()[0], twins[rep])
    assert not bad, bad[:10]


@pytest.mark.gpu
def test_gpu_mesh_pairs_pass_vs_twin(nmi):
    """The two-kernel binning pass (nmi_mesh_cull_kernel + nmi_mesh_bin_pairs_kernel) against the twin.  launch_render_mesh takes
    it when nblocks * views > 4 * compute units: 4,800 triangles are 19 blocks of 256, times 64 views = 1,216 pairs > 4 * 256
    (the test asserts the inequality for the device at hand).  The pass also needs the context's pair list, which
    nmi_render_mesh allocates on demand (ensure_mesh_pairs) and silently does without if the allocation fails: nothing the API
    exposes says which form ran, so this test is the two-kernel pass's only where that allocation succeeded -- 19 x 64 entries."""
    W, H = 160, 120
    views = np.concatenate([rc.shifted(mc.tessellation_views(W, H)[:1], (0.4 * np.sin(0.7 * s), 0.3 * np.cos(1.1 * s), 0.05 * s - 1.0)) for s in range(64)])
    xyz, uv, _ = mc.tessellation_mesh(W, H, views[0], nx=40, ny=30, seed=8)
    xyz, uv = xyz.astype(f32), uv.astype(f32)
    assert len(xyz) // 3 == 4800
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert ((4800 + 255) // 256) * 64 > 4 * cus, cus
    rgb = mc.smooth_texture(100, 60, 9)
    c = {"xyz": xyz, "uv": uv, "rgb": rgb, "mvps": views}
    t0 = time.time()
    staged = twin_stack(c, W, H)
    print(f"twin: {time.time() - t0:.0f} s")
    with nmi.NmiContext(W, H) as ctx, nmi.NmiTexture(ctx, rgb) as tex:
        got, mask = ctx.render_mesh_masked(dev(xyz), dev(uv), tex, views)
        bad = against_twin("pairs pass", got.cpu().numpy(), staged, "pairs_pass") + masks_differ("pairs pass mask", mask.cpu().numpy(), staged)
    print("pairs pass:", DIFFERING.get("pairs_pass"))
    assert not bad, bad[:10]


@pytest.mark.gpu
def test_gpu_huge_uv_is_safe(nmi):
    """uv beyond the wrap's domain on textures with sides that are not powers of two: the renders equal the twin's (whose
    wrap_index is the kernel's, bound included), and an ordinary render on the same context before and after is unchanged."""
    from test_render import plane_mesh
    W, H = 150, 90
    px, pu, prgb, _ = plane_mesh(W, H)
    m = rc.cameras(W, H)["axis"]
    bad = []
    with nmi.NmiContext(W, H) as ctx, nmi.NmiTexture(ctx, prgb) as ptex:
        before = ctx.render_mesh(dev(px), dev(pu), ptex, m[None]).cpu().numpy()
        assert (before != 255).mean() > 0.5
        for i, c in enumerate(mc.family("huge_uv", W, H)):
            assert "beyond_wrap_domain" in mc.branches(c, W, H)
            staged = twin_stack(c, W, H)
            with nmi.NmiTexture(ctx, c["rgb"]) as tex:
                got, mask = ctx.render_mesh_masked(dev(c["xyz"]), dev(c["uv"]), tex, c["mvps"])
                bad += against_twin(f"huge_uv[{i}]", got.cpu().numpy(), staged, "huge_uv") + masks_differ(f"huge_uv[{i}] mask", mask.cpu().numpy(), staged)
        after = ctx.render_mesh(dev(px), dev(pu), ptex, m[None]).cpu().numpy()
    print("huge_uv:", DIFFERING.get("huge_uv"))
    assert (after == before).all()
    assert not bad, bad[:10]
