"""The twin and the float64 model of the vertex-coloured mesh renderer (nmi_render_mesh_colored) -- TEST INFRASTRUCTURE ONLY.

No rasteriser of its own: oracle/mesh_oracle_np.render_staged draws the mesh with attr[:, 0] = colour, attr[:, 1] = 0 and a
one-texel level list; the `u` it returns per pixel IS the interpolated colour by the kernel's arithmetic (the colour takes u's way
through load, near-plane clip, tri_planes and S * (1 / Q)).  Grey = the point renderer's colour rule applied to u in the same
float type, 255 where no fragment won.  F = np.float32 is the twin (bytes the device must equal), F = np.float64 the model.

Colours for the cases of tests/helpers/mesh_cases.py come from a seeded generator, uniform in [-0.1, 1.1] per corner so that both
clamps are reached; the `nonfinite` family also gets NaN and +-inf colours on some corners.
"""
import functools
import zlib

import numpy as np

from helpers import mesh_bounds as mb
from helpers import mesh_cases as mc
from oracle import mesh_oracle_np as mo

f32 = np.float32
ONE_TEXEL = [np.zeros((1, 1), f32)]     # the level list render_staged wants; its sample plays no part


def attr(colors):
    """colours [3T] -> the [3T, 2] attribute array render_staged takes: (colour, 0)."""
    c = np.asarray(colors, f32).reshape(-1)
    return np.ascontiguousarray(np.stack([c, np.zeros_like(c)], 1))


def grey_rule(c, F=f32):
    """(uint32_t)(fminf(fmaxf(c, 0), 1) * 255 + 0.5) in the float type F: fmaxf drops a NaN, so NaN gives 0."""
    c = np.asarray(c, F)
    with np.errstate(all="ignore"):
        return mo.sat_uint(np.fmin(np.fmax(c, F(0.0)), F(1.0)) * F(255.0) + F(0.5))


def render(xyz, colors, mvp, W, H, F=f32):
    """One view -> dict per pixel [H, W]: grey (uint8, 255 where not covered), covered, tri, piece, depth, u (the colour)."""
    st = mo.render_staged(xyz, attr(colors), ONE_TEXEL, mvp, W, H, F)
    grey = np.where(st["covered"], grey_rule(st["u"], F), 255).astype(np.uint8)
    return {"grey": grey, "covered": st["covered"], "tri": st["tri"], "piece": st["piece"], "depth": st["depth"], "u": st["u"]}


def render_stack(xyz, colors, mvps, W, H, F=f32):
    return [render(xyz, colors, m, W, H, F) for m in np.asarray(mvps, f32).reshape(-1, 16)]


@functools.lru_cache(maxsize=None)
def colors_of(family, W, H, i):
    """The seeded colours of case i of a family: float32 [3T], read-only."""
    c = mc.family(family, W, H)[i]
    n = len(c["xyz"])
    rng = np.random.default_rng([zlib.crc32(family.encode()), i, n])
    col = rng.uniform(-0.1, 1.1, n).astype(f32)
    if family == "nonfinite":
        at = rng.choice(n, size=min(n, 9), replace=False)
        col[at] = np.resize(np.array([np.nan, np.inf, -np.inf], f32), len(at))
    col.setflags(write=False)
    return col


@functools.lru_cache(maxsize=None)
def twin_of(family, W, H, i, shift=None):
    """The twin's renders of case i under its own views, or under those views moved by the world translation `shift`."""
    from helpers import render_cases as rc
    c = mc.family(family, W, H)[i]
    mvps = c["mvps"] if shift is None else rc.shifted(c["mvps"], shift)
    return render_stack(c["xyz"], colors_of(family, W, H, i), mvps, W, H)


def compare_view(xyz, colors, m, W, H, bulk=None):
    """The float64 criterion of one view.  Coverage, winner and depth are mesh_bounds.compare_view's business (they do not depend on
    the attribute); its problems that concern them come back as `problems`, with frags / frags_exempt.  The grey is compared on
    exactly the pixels that function compares its own grey on -- a common winner, not exempt for coverage or winner -- with
    E_u = the bound mesh_bounds.shade_ev carries for u there: |grey32 - grey64| <= 255 E_u + 1 (test_mesh_edges' grey criterion
    with the texture's Lipschitz constant replaced by 1: grey = round(255 clamp(u)), and the clamp does not stretch).  Where E_u is
    not finite (fp32 overflow, a NaN colour) the bound says nothing and the pixel is counted as unbounded.
    -> dict: problems, grey_problems, frags, frags_exempt, pixels (compared), unbounded, worst (largest |grey32 - grey64|)."""
    seen = []
    inner = mb.shade_ev

    def recording(s, tu, tv, x_lo, y_lo, xx, yy, tw, th):
        out = inner(s, tu, tv, x_lo, y_lo, xx, yy, tw, th)
        seen.append((np.asarray(yy, np.int64), np.asarray(xx, np.int64), out[0]))
        return out

    mb.shade_ev = recording     # (compare_view calls it once per piece, for the piece's compared pixels)
    try:
        r = mb.compare_view(xyz, attr(colors), ONE_TEXEL, m, W, H, bulk)
    finally:
        mb.shade_ev = inner
    T, M = r["twin"], r["model"]
    g32 = np.where(T["covered"], grey_rule(T["u"], f32), 255).astype(np.int64)
    g64 = np.where(M["covered"], grey_rule(M["u"], np.float64), 255).astype(np.int64)
    grey_problems = []
    n = unbounded = worst = 0
    for yy, xx, u in seen:
        with np.errstate(all="ignore"):
            bound = 255.0 * u.e + 1.0
        fin = np.isfinite(bound)
        d = np.abs(g32[yy, xx] - g64[yy, xx])
        n, unbounded = n + int(fin.sum()), unbounded + int((~fin).sum())
        if fin.any():
            worst = max(worst, int(d[fin].max()))
        bad = fin & (d > bound)
        if bad.any():
            k = int(np.argmax(bad))
            grey_problems.append(f"grey differs by {d[k]} > {bound[k]:.4g} at ({xx[k]}, {yy[k]}); {int(bad.sum())} such pixels")
    own = ("luma", "grey")      # the one-texel texture's: not this renderer's
    return {"problems": [p for p in r["problems"] if not any(k in p for k in own)], "grey_problems": grey_problems, "frags": r["frags"],
            "frags_exempt": r["frags_exempt"], "pixels": n, "unbounded": unbounded, "worst": worst}
