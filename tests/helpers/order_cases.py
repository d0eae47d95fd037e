"""Maps for tests/test_map_order.py: every family of inputs on which the map order (include/nmi_hip.h, "Map order") takes another
branch, as point clouds (verts = 1) and as triangle soups (verts = 3) -- TEST INFRASTRUCTURE ONLY.

case(variant, n, verts) -> dict: xyz [n verts, 3] float32, `disagree`: the records whose placement the float64 model decides
otherwise than fp32 (known by construction: sums that overflow in fp32 alone), `wide`: the axes whose span overflows fp32.
attributes(n, nb) gives every record nb values of its own, so a record whose attributes travelled with other corners shows.

Triangles are built around the points' positions (corners = position + small offsets), except where the family is about the
corners themselves.  A triangle's centroid is at most FLT_MAX / 3 in magnitude when it is finite at all, so a triangle never sits at
the 3.0e38 limit and a soup's span never overflows: for triangles the `limit` variant is about sums that just fit against
sums that overflow, and the `wide` variants are merely very wide.
"""
import functools

import numpy as np

f32 = np.float32
LIMIT = f32(3.0e38)
ABOVE = np.nextafter(LIMIT, f32(np.inf))
FLT_MAX = np.finfo(f32).max
PAYLOAD_NAN = np.array([0xFFC12345], np.uint32).view(f32)[0]          # a negative quiet NaN with a payload

# variant -> the family of the issue it belongs to
VARIANTS = {
    "ordinary": "ordinary", "lattice": "lattice", "extremes": "extremes",
    "identical": "degenerate", "planar": "degenerate", "collinear": "degenerate",
    "zeros": "signed zero and tiny values",
    "nonfinite": "non-finite", "limit": "non-finite", "all_nonfinite": "non-finite", "one_finite": "non-finite",
    "wide": "wide", "nearly_wide": "wide",
    "outlier": "outlier", "ties": "ties",
}

# Record counts.  1 and 2 are the degenerate family's "n = 1" and "two records"; 63 .. 257 straddle a wavefront and a workgroup of
# the three kernels.
SMALL = (1, 2, 63, 64, 65, 255, 256, 257, 1000)
# nmi_box_kernel runs at most 2,048 workgroups of 256: from 524,289 records on its threads take the stride loop.
STRIDE = (2048 * 256 + 4321,)
# rocprim::radix_sort_pairs (rocPRIM 4.2.0, rocprim/device/device_radix_sort.hpp, radix_sort_impl, uint32 keys and values, default
# config) has three forms:
#   size <= 1,024          one block: radix_sort_block_sort, kernel_config<min(256, .), min(4, .)> = 256 threads x 4 items
#   size <= 1,048,576      radix_sort_merge_impl (radix_sort_config<>::merge_sort_limit = 1024 * 1024), inside which
#                          device_merge_sort.hpp merges odd-even up to merge_oddeven_config.size_limit = (1 << 17) + 70000 =
#                          201,072 items (every gfx9 entry of detail/config/device_merge_sort_block_merge.hpp and the default) and
#                          by merge path above
#   larger                 radix_sort_onesweep_impl (multi-pass)
# 2,048 is what one block of the merge form's block sort holds by the untuned default (merge_sort_block_sort_config_base: 256 threads
# x 8 items for 4-byte items); whether the tuned table of the device at hand keeps that figure was not established, the pair is
# cheap and stays.
SWITCH = (1024, 1025, 2048, 2049, 201072, 201073, 1048576, 1048577)
COUNTS = SMALL + SWITCH + STRIDE

BOX_LO = np.array([-30.0, -5.0, -8.0], f32)       # off-centre, with negative coordinates
BOX_HI = np.array([10.0, 25.0, 4.0], f32)


def attributes(n, nb):
    """[n, nb] float32: value nb i + k for record i (exact below 2^24), the index planted; one -0.0 and one NaN with a payload, so
    that the comparison of bits has some to tell apart."""
    assert n * nb < 2 ** 24
    b = (np.arange(n, dtype=np.int64)[:, None] * nb + np.arange(nb)).astype(f32)
    if n > 3:
        b[n // 2, 0] = f32(-0.0)
        b[n // 3, -1] = PAYLOAD_NAN
    return b


def _cloud(rng, n, lo=BOX_LO, hi=BOX_HI):
    return (lo + (hi - lo) * rng.random((n, 3), dtype=f32)).astype(f32)


def _triangles(P, rng, size, axes=(1, 1, 1)):
    """Corners [n, 3, 3] around the positions P: position + size * offsets in [-1, 1) on the given axes."""
    d = (rng.random((len(P), 3, 3), dtype=f32) * f32(2) - f32(1)) * f32(size) * np.asarray(axes, f32)
    with np.errstate(all="ignore"):
        return (P[:, None, :] + d).astype(f32)


def _put(a, i, value):
    if 0 <= i < len(a):
        a[i] = value
        return True
    return False


@functools.lru_cache(maxsize=4)
def case(variant, n, verts):
    rng = np.random.default_rng(abs(hash((sorted(VARIANTS).index(variant), n, verts))) % (2 ** 32))
    size, axes = 0.25, (1, 1, 1)
    disagree, wide = [], (False, False, False)
    corners = None
    if variant == "ordinary":
        P = _cloud(rng, n)
        _put(P, n - 2, BOX_LO - f32(1)), _put(P, n - 1, BOX_HI + f32(1))       # the box is defined by the last records
    elif variant == "lattice":
        lo, span = np.array([-3.5, 2.25, -100.0]), np.array([7.3, 0.011, 250.0])
        i = np.arange(n)
        j = np.stack([(i * 1 + 0) % 1024, (i * 341 + 7) % 1024, (i * 683 + 100) % 1024], 1)
        if n > 1:
            j[0], j[1] = 0, 1023
        P = (lo + j * span / 1023.0).astype(f32)
        lo32, hi32 = lo.astype(f32), (lo + span).astype(f32)
        side = (i % 3)[:, None]
        P = np.where(side == 1, np.nextafter(P, f32(np.inf)), np.where(side == 2, np.nextafter(P, f32(-np.inf)), P))
        P = np.clip(P, lo32, hi32).astype(f32)
        size = 0.0
    elif variant == "extremes":
        P = _cloud(rng, n, BOX_LO * f32(0.5), BOX_HI * f32(2))
        for k in range(3):                                                     # one record per face of the box, at the end
            for s, edge in enumerate((BOX_LO * f32(0.5) - f32(2), BOX_HI * f32(2) + f32(2))):
                if n - 1 - (2 * k + s) >= 0:
                    P[n - 1 - (2 * k + s), k] = edge[k]
    elif variant == "identical":
        P = np.tile(np.array([1.5, -2.25, 1e-3], f32), (n, 1))
        size = 0.0
    elif variant == "planar":
        P = _cloud(rng, n)
        P[:, 2] = f32(0.1)
        axes = (1, 1, 0)
    elif variant == "collinear":
        P = _cloud(rng, n)
        P[:, 1], P[:, 2] = f32(-0.3), f32(7.0)
        axes = (1, 0, 0)
    elif variant == "zeros":
        tiny = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-40, -1e-40, 1.1754942e-38, -1.1754942e-38, 1.17549435e-38, -1.17549435e-38], f32)
        P = np.stack([np.array([0.0, -0.0], f32)[rng.integers(0, 2, n)], tiny[rng.integers(0, len(tiny), n)],
                      np.array([-0.0, 0.0, 1.0], f32)[rng.integers(0, 3, n)]], 1)
        size = 0.0
    elif variant in ("nonfinite", "all_nonfinite", "one_finite"):
        P = _cloud(rng, n)
        corners = _triangles(P, rng, size) if verts == 3 else P[:, None, :].copy()
        specials = np.array([np.nan, np.inf, -np.inf, PAYLOAD_NAN], f32)
        i = np.arange(n)
        hit = (i % 7 == 0) if variant == "nonfinite" else np.ones(n, bool)
        if variant == "one_finite":
            hit[n // 2] = False
        r = np.nonzero(hit)[0]
        corners[r, r % verts, (r // 7) % 3] = specials[(r // 21) % 4]
    elif variant == "limit":
        P = _cloud(rng, n)
        if verts == 1:
            step = max(n // 7, 1)
            for s, (k, value) in enumerate([(0, LIMIT), (0, ABOVE), (0, FLT_MAX), (1, -LIMIT), (1, -ABOVE), (2, -FLT_MAX)]):
                if s * step < n:
                    P[s * step, k] = value
        else:
            corners = _triangles(P, rng, size)
            step = max(n // 8, 1)
            # (axis, the three corners' coordinates, fp32 places it, the model places it)
            rows = [(0, (1.7e38, 1.7e38, 0.0), True, True),                    # the sum just fits: 3.4e38
                    (0, (1.7015e38, 1.7015e38, 0.0), False, True),             # p0 + p1 overflows
                    (0, (FLT_MAX, FLT_MAX, -FLT_MAX), False, True),
                    (1, (-1.7e38, -1.7e38, 0.0), True, True),
                    (1, (-3e38, -3e38, 3e38), False, True),
                    (2, (-FLT_MAX, 0.0, 0.0), True, True),
                    (0, (1.5e38, 1.5e38, 1e38), False, True)]                  # (p0 + p1) + p2 overflows
            for s, (k, vals, in32, in64) in enumerate(rows):
                if s * step < n:
                    corners[s * step, :, k] = np.array(vals, f32)
                    if in32 != in64:
                        disagree.append(s * step)
    elif variant in ("wide", "nearly_wide"):
        P = _cloud(rng, n)
        if verts == 1:
            ends = (LIMIT, f32(2.5e38), f32(2e38)) if variant == "wide" else (f32(1.7e38), f32(2.5e38), None)
        else:
            ends = (f32(1.1e38), f32(1.0e38), f32(0.9e38)) if variant == "wide" else (f32(1.1e38), f32(0.6e38), None)
            corners = _triangles(P, rng, size)
        if n > 1:
            for k, e in enumerate(ends):
                if e is not None:
                    if corners is None:
                        P[0, k], P[n - 1, k] = -e, e
                    else:
                        corners[0, :, k], corners[n - 1, :, k] = -e, e
            if verts == 1:
                wide = (True, True, True) if variant == "wide" else (False, True, False)
    elif variant == "outlier":
        P = _cloud(rng, n)
        _put(P, n // 3, np.array([1e6, -1e6, 1e6], f32))
    elif variant == "ties":
        span = BOX_HI - BOX_LO
        P = (BOX_LO + span * np.array([0.37, 0.6104, 0.8303], f32) + span / f32(1023 * 4) * rng.random((n, 3), dtype=f32)).astype(f32)
        _put(P, 0, BOX_LO), _put(P, n - 1, BOX_HI)
        size = 1e-4
    else:
        raise KeyError(variant)
    if corners is None:
        corners = _triangles(P, rng, size, axes) if verts == 3 and size else np.repeat(P[:, None, :], verts, 1)
    xyz = np.ascontiguousarray(corners.reshape(n * verts, 3), f32)
    xyz.setflags(write=False)
    return {"xyz": xyz, "disagree": sorted(disagree), "wide": wide, "n": n, "verts": verts, "variant": variant}
