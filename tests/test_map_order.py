"""The map order of nmi_sort_points / nmi_sort_triangles / nmi_sort_triangles_colored (csrc/nmi_sort.hip), record for record.

The rule is written in include/nmi_hip.h ("Map order"): key, then input index.  tests/helpers/morton_np.py restates it in
np.float32 (the twin) and in float64 (the model) and derives the bound B on |t 1023 (fp32) - t 1023 (float64)|;
tests/helpers/order_cases.py builds the maps.

CPU tier: the twin's cell lies in [floor(v - B), floor(v + B)] of the model's v = t 1023 -- where v is farther than B from an
integer that is the model's cell, nearer it is one of the two adjacent cells; placement (|c| <= 3.0e38) is decided alike except on
the records the cases list; the interleave is fixed by literal keys.  GPU tier: both output arrays of every call equal
input[order(keys(input))] on every bit; a context's second call equals a fresh context's; overlapping and null arguments are
refused with the outputs untouched; levels render and score a map, the sorted map and the reversed sorted map alike.

Observed on the CPU (test_exemption_cap, 200,000 records): the ordinary family has 0.147 % of its points and 0.424 % of its
triangles within B of a cell border on some axis (expected for points: 3 axes x 2 sides x POINT_BOUND 2.44e-4 = 0.146 %); on the
lattice family it is every record but one, points and triangles alike.
"""
import functools

import numpy as np
import pytest

from helpers import morton_np as mn
from helpers import order_cases as oc

try:
    import torch
except ImportError:  # the CPU tier does not need it
    torch = None

f32 = np.float32
CPU_COUNTS = oc.SMALL + (1025, 4099)
FORMS = {"points": (1, 3, 1), "textured": (3, 9, 6), "colored": (3, 9, 3)}      # verts, floats per record of a, of b
W, H = 64, 48


def bits(a):
    return np.ascontiguousarray(a, f32).reshape(-1).view(np.uint32)


# ----------------------------------------------------------------------------------------------------- CPU tier
def compare(c):
    """Twin against model on one case -> (records exempt on some axis, placed records)."""
    xyz, verts, tag = c["xyz"], c["verts"], f"{c['variant']} n={c['n']} verts={c['verts']}"
    cell32, ok32 = mn.cells(xyz, verts)
    c64 = mn.positions(xyz, verts, np.float64)
    ok64 = mn.placed(c64)
    # placement: alike, except the listed records, whose sum overflows in fp32 alone
    differ = np.nonzero(ok32 != ok64)[0]
    assert list(differ) == c["disagree"], f"{tag}: placement differs at {differ[:8]}, expected {c['disagree']}"
    for i in differ:
        assert not np.isfinite(mn.positions(xyz, verts)[i]).all() and ok64[i] and not ok32[i], f"{tag}: record {i} is not an fp32-only overflow"
    with np.errstate(all="ignore"):
        e_c = mn.bound(xyz, verts, ok32)[1]
        near_limit = (np.isfinite(c64) & (e_c > 0) & (np.abs(np.abs(c64) - float(mn.LIMIT)) <= e_c)).any(1)
    assert not near_limit.any(), f"{tag}: a centroid within its bound of 3.0e38: list it"
    # cells, on the twin's placement
    cell64, v, _, wide = mn.cells64(xyz, verts, ok32)
    assert tuple(bool(x) for x in wide) == tuple(c["wide"]), f"{tag}: wide axes {wide}"
    B, _ = mn.bound(xyz, verts, ok32)
    first, last = mn.allowed_cells(v, B)
    first[:, wide], last[:, wide] = 0, 0
    bad = ok32[:, None] & ((cell32 < first) | (cell32 > last))
    assert not bad.any(), (f"{tag}: {int(bad.sum())} cells outside the model's range, first record {np.nonzero(bad.any(1))[0][0]}: "
                           f"twin {cell32[bad][:3]}, model v {v[bad][:3]}, bound {B[bad][:3]}")
    decided = first == last
    assert (cell32[decided & ok32[:, None]] == cell64[decided & ok32[:, None]]).all()        # (what the range says, spelled out)
    assert (last - first <= 1)[np.isfinite(B) & (B < 0.5)].all()
    assert (cell32[~ok32] == 0).all()
    return int((~decided & ok32[:, None]).any(1).sum()), int(ok32.sum())


@pytest.mark.parametrize("verts", [1, 3], ids=["points", "triangles"])
@pytest.mark.parametrize("variant", list(oc.VARIANTS))
def test_twin_meets_float64_model(variant, verts):
    exempt = total = 0
    for n in CPU_COUNTS:
        c = oc.case(variant, n, verts)
        e, t = compare(c)
        exempt, total = exempt + e, total + t
        k = mn.keys(c["xyz"], verts)
        o = mn.order(k)
        _, ok = mn.cells(c["xyz"], verts)
        assert (k[~ok] == 0x40000000).all() and (k[ok] < 0x40000000).all()
        assert ok[o[:ok.sum()]].all() and (np.diff(o[ok.sum():]) > 0).all()          # not placed: last, in input order
        assert ((np.diff(k[o]) > 0) | (np.diff(o) > 0)).all()                      # equal keys: input order
        if variant in ("identical", "all_nonfinite") or (variant == "wide" and verts == 1):
            assert (o == np.arange(n)).all(), "the output is not the input order"
        if variant == "one_finite":
            assert o[0] == n // 2 and k[n // 2] == 0
        if variant == "limit" and n >= 7 and verts == 1:
            step = n // 7
            assert list(ok[[0, step, 2 * step, 3 * step, 4 * step, 5 * step]]) == [True, False, False, True, False, False]
    print(f"{variant} verts={verts}: {exempt} of {total} placed records within the bound of a cell border")


@pytest.mark.parametrize("verts", [1, 3], ids=["points", "triangles"])
def test_box_defining_records_get_cells_0_and_1023(verts):
    for variant in ("extremes", "ordinary", "outlier", "lattice"):
        for n in CPU_COUNTS[1:]:
            c = oc.case(variant, n, verts)
            cell, ok = mn.cells(c["xyz"], verts)
            p = mn.positions(c["xyz"], verts)
            for k in range(3):
                lo, hi = p[ok, k].min(), p[ok, k].max()
                if hi > lo:
                    assert (cell[ok & (p[:, k] == lo), k] == 0).all() and (cell[ok & (p[:, k] == hi), k] == 1023).all()
    c = oc.case("extremes", 1000, verts)            # every face of the box has its record among the last six
    p = mn.positions(c["xyz"], verts)
    assert set(np.argmin(p, 0)) | set(np.argmax(p, 0)) == set(range(994, 1000))


def test_exemption_cap():
    """Ordinary family: below 1 % of the records are within the bound of a cell border on some axis (observed: 294 of 200,000
    points, 0.147 %, and 848 of 200,000 triangles, 0.424 %).  Lattice family: the exemption occurs (observed: 199,999 of 200,000
    records, points and triangles alike), or the family would not reach its branch."""
    for verts in (1, 3):
        e, t = compare(oc.case("ordinary", 200000, verts))
        print(f"ordinary verts={verts}: {e} of {t} records exempt ({100.0 * e / t:.3f} %)")
        assert t == 200000 and e < 0.01 * t
        e, t = compare(oc.case("lattice", 200000, verts))
        print(f"lattice verts={verts}: {e} of {t} records exempt ({100.0 * e / t:.1f} %)")
        assert e > 0.1 * t
    assert mn.POINT_BOUND < 2.5e-4
    B, _ = mn.bound(oc.case("ordinary", 1000, 1)["xyz"], 1)
    assert (B <= mn.POINT_BOUND).all() and (B > 0.9 * mn.POINT_BOUND).all()


@pytest.mark.parametrize("verts", [1, 3], ids=["points", "triangles"])
def test_interleave_literal_keys(verts):
    """The bit order by numbers: x is bit 0 of every triple, y bit 1, z bit 2; cell bit b is key bit 3 b + axis."""
    rows = [((0, 0, 0), 0), ((1023, 1023, 1023), 0x3FFFFFFF),
            ((1.5, 0, 0), 1), ((0, 1.5, 0), 2), ((0, 0, 1.5), 4),
            ((2.5, 0, 0), 8), ((0, 2.5, 0), 16), ((0, 0, 2.5), 32),
            ((512.5, 0, 0), 1 << 27), ((0, 512.5, 0), 1 << 28), ((0, 0, 512.5), 1 << 29),
            ((1023, 0, 0), 0x09249249), ((0, 1023, 0), 0x12492492), ((0, 0, 1023), 0x24924924),
            ((682.5, 0, 341.5), 0x08208208 | 0x04104104),                # x = 0b1010101010, z = 0b0101010101
            ((np.nan, 0, 0), 0x40000000), ((0, np.inf, 0), 0x40000000), ((0, 0, 3.1e38), 0x40000000)]
    P = np.array([r[0] for r in rows], f32)
    k = mn.keys(np.repeat(P, verts, 0), verts)
    assert [int(x) for x in k] == [r[1] for r in rows]
    assert mn.interleave(np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1023]])).tolist() == [1, 2, 0x24924924]


# ----------------------------------------------------------------------------------------------------- GPU tier
@pytest.fixture(scope="module")
def nmi():
    if torch is None or not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    import orbslam2_nmi_amd as m
    m.load_library()
    return m


@pytest.fixture(scope="module")
def ctx(nmi):
    with nmi.NmiContext(W, H) as c:
        yield c


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()       # (a copy: the cases are read-only)


@functools.lru_cache(maxsize=4)
def expected(variant, n, verts):
    """-> (a [n, 3 verts] float32, order) of the case, computed once for the forms that share it."""
    xyz = oc.case(variant, n, verts)["xyz"]
    return xyz.reshape(n, 3 * verts), mn.order(mn.keys(xyz, verts))


def device_sort(ctx, form, a, b):
    """One call of the form's entry on host arrays a [n, na], b [n, nb] -> the two outputs as host arrays of those shapes."""
    n = len(a)
    if form == "points":
        xo, bo = ctx.sort_points(dev(a), dev(b.reshape(n)))
    elif form == "textured":
        xo, bo = ctx.sort_triangles(dev(a.reshape(3 * n, 3)), dev(b.reshape(3 * n, 2)))
    else:
        xo, bo = ctx.sort_triangles_colored(dev(a.reshape(3 * n, 3)), dev(b.reshape(3 * n)))
    return xo.cpu().numpy().reshape(a.shape), bo.cpu().numpy().reshape(b.shape)


def order_problems(tag, a, b, o, got_a, got_b):
    bad = []
    for name, want, got in (("positions", a[o], got_a), ("attributes", b[o], got_b)):
        d = (bits(want) != bits(got)).reshape(len(a), -1).any(1)
        if d.any():
            i = int(np.nonzero(d)[0][0])
            bad.append(f"{tag}: {name} differ at {int(d.sum())} of {len(a)} output records, first {i}: got {got[i]}, twin {want[i]} (input record {o[i]})")
    return bad


ORDER_CASES = [(v, n, f) for v in oc.VARIANTS for n in oc.COUNTS for f in FORMS]


@pytest.mark.gpu
@pytest.mark.parametrize("variant,n,form", ORDER_CASES, ids=[f"{v}-{n}-{f}" for v, n, f in ORDER_CASES])
def test_gpu_exact_order(ctx, variant, n, form):
    """Both outputs equal input[order(keys(input))] on every bit (uint32 views: NaN payloads and -0.0 count)."""
    verts, na, nb = FORMS[form]
    a, o = expected(variant, n, verts)
    b = oc.attributes(n, nb)
    got_a, got_b = device_sort(ctx, form, a, b)
    bad = order_problems(f"{variant} n={n} {form}", a, b, o, got_a, got_b)
    assert not bad, bad


@pytest.mark.gpu
@pytest.mark.parametrize("form", list(FORMS))
def test_gpu_second_call_equals_fresh_context(nmi, form):
    """Larger, then smaller, across the radix sort's three forms, on one context: every call gives what a fresh context gives (and
    the twin): nothing is left over in temporary storage."""
    verts, na, nb = FORMS[form]
    counts = (1000, 1048577, 201073, 257, 2049, 1)
    bad = []
    with nmi.NmiContext(W, H) as used:
        for n in counts:
            a, o = expected("ordinary", n, verts)
            b = oc.attributes(n, nb)
            got = device_sort(used, form, a, b)
            with nmi.NmiContext(W, H) as fresh:
                ref = device_sort(fresh, form, a, b)
            if not ((bits(got[0]) == bits(ref[0])).all() and (bits(got[1]) == bits(ref[1])).all()):
                bad.append(f"n={n}: the used context's result differs from a fresh context's")
            bad += order_problems(f"n={n} {form}", a, b, o, *got)
    assert not bad, bad


@pytest.mark.gpu
@pytest.mark.parametrize("form", list(FORMS))
def test_gpu_rejections_leave_the_outputs_untouched(ctx, form):
    """NMI_ERR_INVALID_ARGUMENT before anything is touched: outputs overlapping an input or each other at offsets of one record and
    of n - 1 records, in both directions and across the two arrays; null pointers; n < 0; n = 2^32 with one-element buffers.
    n = 0 is NMI_OK with null pointers.  Arrays that merely touch are accepted and sorted."""
    from orbslam2_nmi_amd import capi
    verts, na, nb = FORMS[form]
    fn = {"points": ctx._lib.nmi_sort_points, "textured": ctx._lib.nmi_sort_triangles, "colored": ctx._lib.nmi_sort_triangles_colored}[form]
    h, E = ctx._h, capi.ERR_INVALID_ARGUMENT
    n = 100
    a, o = expected("ordinary", n, verts)
    b = oc.attributes(n, nb)
    ra, rb = 4 * na, 4 * nb                                   # bytes per record
    slot = 4 * n * (na + nb)                                  # bytes: room for either array
    pool = torch.full((8 * slot // 4,), 7.0, dtype=torch.float32, device="cuda")
    base = pool.data_ptr()
    A, Bp, AO, BO = base + 2 * slot, base + 4 * slot, base + 5 * slot + slot // 2, base + 7 * slot     # far apart
    pool[(A - base) // 4:(A - base) // 4 + n * na] = dev(a).reshape(-1)
    pool[(Bp - base) // 4:(Bp - base) // 4 + n * nb] = dev(b).reshape(-1)
    keep = pool.clone()
    torch.cuda.synchronize()
    calls = []
    for d in (1, n - 1):
        calls += [(A + d * ra, BO), (A - d * ra, BO), (AO, Bp + d * rb), (AO, Bp - d * rb)]                 # an output on its own input
        calls += [(Bp + d * rb, BO), (Bp - d * ra, BO), (AO, A + d * ra), (AO, A - d * rb)]                 # ... on the other input
        calls += [(AO, AO + d * ra), (AO, AO - d * rb)]                                                      # ... on the other output
    calls += [(A, BO), (AO, Bp)]                                                                             # pointer equality
    for ao, bo in calls:
        assert fn(h, A, Bp, n, ao, bo) == E, (ao - base, bo - base)
    for args in ((None, Bp, AO, BO), (A, None, AO, BO), (A, Bp, None, BO), (A, Bp, AO, None)):
        assert fn(h, args[0], args[1], n, args[2], args[3]) == E
    assert fn(h, A, Bp, -1, AO, BO) == E
    assert fn(h, A, Bp, 1 << 32, AO, BO) == E
    one = torch.full((4,), 7.0, dtype=torch.float32, device="cuda")
    assert fn(h, one.data_ptr(), one.data_ptr() + 4, 1 << 32, one.data_ptr() + 8, one.data_ptr() + 12) == E
    assert fn(None, A, Bp, n, AO, BO) == E
    assert fn(h, None, None, 0, None, None) == capi.NMI_OK
    ctx.synchronize()
    torch.cuda.synchronize()
    assert torch.equal(pool.view(torch.int32), keep.view(torch.int32)) and (one == 7).all()
    # arrays that touch but share no byte: a | a_out | b_out | b in one run of memory
    run = torch.full((2 * n * (na + nb),), 7.0, dtype=torch.float32, device="cuda")
    r0 = run.data_ptr()
    run[:n * na] = dev(a).reshape(-1)
    run[n * (2 * na + nb):] = dev(b).reshape(-1)
    torch.cuda.synchronize()
    assert fn(h, r0, r0 + 4 * n * (2 * na + nb), n, r0 + 4 * n * na, r0 + 4 * n * 2 * na) == capi.NMI_OK
    got = run.cpu().numpy()
    bad = order_problems(f"touching arrays {form}", a, b, o, got[n * na:2 * n * na].reshape(n, na), got[2 * n * na:n * (2 * na + nb)].reshape(n, nb))
    assert not bad, bad
    assert (bits(got[:n * na]) == bits(a)).all() and (bits(got[n * (2 * na + nb):]) == bits(b)).all()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["cloud", "textured", "colored"])
def test_gpu_levels_do_not_see_the_order(nmi, kind):
    """A level over the map as given, over the map after nmi_sort_* and over the sorted map reversed, S = 3, Wn = 3, two replays
    each: the same renders, the same bits in the rating table, the same winner.  (The consumers the order exists for: the packed
    cloud's 64-point boxes, the kept list, the mesh block cull.)"""
    from test_masked_level import Scene, views, warps
    from test_render import plane_mesh
    S, Wn = 3, 3
    with nmi.NmiContext(W, H) as c:
        if kind == "colored":
            xyz, _, _, rp = plane_mesh(W, H, nx=12, ny=9)
            col = (0.5 + 0.45 * np.sin(3.0 * xyz[:, 0]) * np.cos(2.0 * xyz[:, 1])).astype(f32)     # one colour per place: corners that meet agree
            dx, da, tex = dev(xyz), dev(col), None
            from orbslam2_nmi_amd import capi
            from test_masked_level import camera
            fr = c.render_mesh_colored(dx, da, capi.render_mvp(rp, *camera(), (0.05, 0, 0))[None])[0]
            frame = torch.flip(fr, dims=[0]).contiguous()
            sort, na, nb = c.sort_triangles_colored, 9, 3
        else:
            sc = Scene(nmi, c, W, H, kind == "textured")
            dx, da, tex, frame, rp = sc.dx, sc.da, sc.tex, sc.frame, sc.rp
            sort, na, nb = (c.sort_triangles, 9, 6) if kind == "textured" else (c.sort_points, 3, 1)
        n = dx.numel() // na
        sx, sa = sort(dx, da)
        assert not torch.equal(sx, dx), "the map was in Morton order already"
        rx = sx.reshape(n, na).flip(0).contiguous().reshape(dx.shape)
        ra = sa.reshape(n, nb).flip(0).contiguous().reshape(da.shape)
        replays = [(views(rp, S), warps(W, H, Wn)), (views(rp, S, 1.7), warps(W, H, Wn, 1.6))]
        results = []
        for x, a in ((dx, da), (sx, sa), (rx, ra)):
            with nmi.NmiLevel(c, x, a, frame, S, Wn, 3.0, texture=tex, colors=kind == "colored") as lv:
                out = []
                for mvps, Ms in replays:
                    win = lv.run(mvps, Ms)
                    r, v, t = lv.outputs()
                    out.append((win[0], np.float32(win[1]).view(np.uint32), r, v, t.view(np.uint32)))
                results.append(out)
        assert (results[0][0][2] != 255).mean() > 0.3, "the renders are nearly empty"
        assert len(np.unique(results[0][0][4])) > S * Wn // 2, "the ratings do not tell the cells apart"
        for name, res in (("sorted", results[1]), ("reversed", results[2])):
            for rep, (g, w) in enumerate(zip(results[0], res)):
                assert (g[2] == w[2]).all(), f"{kind} {name} replay {rep}: {int((g[2] != w[2]).sum())} render pixels differ"
                assert (g[3] == w[3]).all()
                assert (g[4] == w[4]).all(), f"{kind} {name} replay {rep}: rating bits differ"
                assert g[0] == w[0] and g[1] == w[1], f"{kind} {name} replay {rep}: winner {w[:2]} != {g[:2]}"
