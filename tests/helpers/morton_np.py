"""The map order of nmi_sort_points / nmi_sort_triangles / nmi_sort_triangles_colored (include/nmi_hip.h, "Map order") in numpy
-- TEST INFRASTRUCTURE ONLY.

keys() is the twin: the header's rule in np.float32, operation for operation (the library is compiled with -ffp-contract=off and
the compiler's default fp32 division is the correctly rounded one, so numpy's float32 is the same arithmetic).  order() is the
order the rule implies: key, then input index.  cells64() is the model: the same cells from float64 positions, box and
quotient.  bound() is the derived bound on |t 1023 (fp32) - t 1023 (float64)| that tells where the two must agree.

Derivation of the bound (standard model: fl(a o b) = (a o b)(1 + d), |d| <= u = 2^-24, plus 2^-149 where a quotient or product is
subnormal; sums and differences that are subnormal are exact).  Per axis, with S = hi - lo of the float64 box and a_k = |p_k|:
  centroid   s1 = fl(p0 + p1), s2 = fl(s1 + p2), c^ = fl(s2 / 3):
                 |s2 - (p0 + p1 + p2)| <= u (a0 + a1) + u ((1 + u)(a0 + a1) + a2) <= (2u + u^2)(a0 + a1 + a2)
                 |c^ - c| <= [(2u + u^2) + u (1 + 2u + u^2)] (a0 + a1 + a2) / 3 + 2^-149 <= (3u + 4u^2)(a0 + a1 + a2) / 3 + 2^-149 =: e_c
             (a point is its own position: e_c = 0)
  box        min and max do not stretch: |lo^ - lo|, |hi^ - hi| <= E := the largest e_c among the placed records
  numerator  n^ = fl(c^ - lo^), |c^ - lo^| <= S + 2E:      |n^ - (c - lo)| <= e_c + E + u (S + 2E) =: e_n
  span       d^ = fl(hi^ - lo^):                           |d^ - S| <= 2E + u (S + 2E) =: e_d
  quotient   q^ = fl(n^ / d^), n^ <= d^ so q^ <= 1:        |q^ - t| <= (e_n + t e_d) / (S - e_d) + u + 2^-149, t <= 1
  clamp      to [0, 1] does not stretch
  product    v^ = fl(q^ 1023):                             |v^ - 1023 t| <= 1023 ((e_n + e_d) / (S - e_d) + u) + 1023 u + 2^-149
So  B = 1023 ((e_n + e_d) / (S - e_d) + 2u) + 2^-148, infinite where S <= e_d, and 0 where S = 0 (the cell is 0 by the rule).
For points e_n = e_d = u S and B = 1023 (2u / (1 - u) + 2u) <= POINT_BOUND = 1023 * 4u (1 + 2^-19) = 2.44e-4 whatever the
box: six cell borders' worth of it (3 axes, both sides) is 0.15 % of a uniform cloud.  Nothing here is fitted to what the twin
gives.
"""
import numpy as np

f32 = np.float32
U = 2.0 ** -24
TINY = 2.0 ** -149
LIMIT = f32(3.0e38)                         # "placed": |c| <= 3.0e38f on every axis
UNPLACED_KEY = np.uint32(0x40000000)
FLT_MAX = np.finfo(f32).max
OVERFLOW = 2.0 ** 128 - 2.0 ** 103          # a float64 value rounds to an fp32 infinity from here on (nearest-even)
POINT_BOUND = 1023 * 4 * U * (1 + 2.0 ** -19)


def positions(xyz, verts, dtype=f32):
    """Records' positions [n, 3]: the point, or ((p0 + p1) + p2) / 3 of `verts` = 3 consecutive corners, in `dtype`."""
    p = np.ascontiguousarray(xyz, f32).reshape(-1, verts, 3).astype(dtype)
    with np.errstate(all="ignore"):
        c = p[:, 0]
        for v in range(1, verts):
            c = c + p[:, v]
        if verts > 1:
            c = c / dtype(verts)
    return c


def placed(c):
    """[n] bool: all three coordinates have |c| <= 3.0e38f (a NaN compares false)."""
    with np.errstate(all="ignore"):
        return (np.abs(c) <= c.dtype.type(LIMIT)).all(1)


def interleave(cells):
    """cells [n, 3] uint32 (10 bits each) -> keys [n]: bit 3 b + k of the key is bit b of axis k's cell."""
    cells = np.asarray(cells, np.uint32)
    key = np.zeros(len(cells), np.uint32)
    for k in range(3):
        for b in range(10):
            key |= ((cells[:, k] >> np.uint32(b)) & np.uint32(1)) << np.uint32(3 * b + k)
    return key


def cells(xyz, verts):
    """The twin's cells [n, 3] uint32 (0 for records that are not placed) and the placed mask [n]."""
    c = positions(xyz, verts)
    ok = placed(c)
    out = np.zeros(c.shape, np.uint32)
    if ok.any():
        with np.errstate(all="ignore"):
            lo, hi = c[ok].min(0), c[ok].max(0)
            span = hi - lo
            t = np.where(span > f32(0), (c - lo) / span, f32(0)).astype(f32)
            t = np.fmin(np.fmax(t, f32(0)), f32(1))                      # fmaxf / fminf: a NaN gives the other operand
            v = t * f32(1023.0)
        assert v.dtype == f32
        out[ok] = v[ok].astype(np.uint32)
    return out, ok


def keys(xyz, verts):
    """The twin: keys [n] uint32 of the records of xyz (verts = 1: points [n, 3]; 3: corners [3 n, 3])."""
    cl, ok = cells(xyz, verts)
    return np.where(ok, interleave(cl), UNPLACED_KEY).astype(np.uint32)


def order(keys_):
    """Input indices in output order: by key, equal keys in input order."""
    return np.argsort(keys_, kind="stable")


def cells64(xyz, verts, placed_mask=None):
    """The model: cells [n, 3] int64 from float64 positions, box and quotient, their values v = t 1023 [n, 3], the placed mask
    and `wide` [3]: axes whose span overflows fp32 (cell 0 for every record, by the rule).  placed_mask: take this placement
    instead of the model's own (for maps on which the two are known to differ)."""
    c = positions(xyz, verts, np.float64)
    ok = placed(c) if placed_mask is None else np.asarray(placed_mask, bool)
    v = np.zeros(c.shape)
    wide = np.zeros(3, bool)
    if ok.any():
        with np.errstate(all="ignore"):
            lo, hi = c[ok].min(0), c[ok].max(0)
            span = hi - lo
            wide = span >= OVERFLOW
            t = np.where((span > 0) & ~wide, (c - lo) / np.where(span > 0, span, 1.0), 0.0)
            v = np.where(ok[:, None], np.clip(t, 0.0, 1.0) * 1023.0, 0.0)
    return np.floor(v).astype(np.int64), v, ok, wide


def bound(xyz, verts, placed_mask=None):
    """B [n, 3] of the module's docstring (inf on an axis whose span is within its own error), and e_c [n, 3]."""
    p = np.ascontiguousarray(xyz, f32).reshape(-1, verts, 3).astype(np.float64)
    c = positions(xyz, verts, np.float64)
    ok = placed(c) if placed_mask is None else np.asarray(placed_mask, bool)
    with np.errstate(all="ignore"):
        e_c = (3 * U + 4 * U * U) * np.abs(p).sum(1) / 3 + TINY if verts > 1 else np.zeros(c.shape)
        if not ok.any():
            return np.zeros(c.shape), e_c
        E = e_c[ok].max(0)
        S = c[ok].max(0) - c[ok].min(0)
        e_d = 2 * E + U * (S + 2 * E)
        e_n = e_c + E + U * (S + 2 * E)
        B = 1023 * ((e_n + e_d) / np.where(S > e_d, S - e_d, 1.0) + 2 * U) + 2 * TINY
        B = np.where(S > e_d, B, np.inf)
        B = np.where(S == 0, 0.0, B) * (1 + 2.0 ** -20)
    return np.where(ok[:, None], B, 0.0), e_c


def allowed_cells(v, B):
    """Per record and axis the closed range of cells a value within B of v can truncate to: (first, last) int64 [n, 3]."""
    with np.errstate(all="ignore"):
        lo = np.where(np.isfinite(B), np.floor(np.clip(v - B, 0.0, 1023.0)), 0.0)
        hi = np.where(np.isfinite(B), np.floor(np.clip(v + B, 0.0, 1023.0)), 1023.0)
    return lo.astype(np.int64), hi.astype(np.int64)
