"""Planted histograms for the data-dependent tone maps (PERCENTILE, EQUALIZE; rule: include/nmi_hip.h "Deep frames", kernels:
csrc/nmi_tone.hip) -- TEST INFRASTRUCTURE ONLY.

What decides a branch of the table scan is the frame's histogram, so a case here is a histogram, not a picture: a sparse
{raw value: count} dict (raw values above M = 2^bits - 1 saturate into h[M]), the bits and the tone map.  frame_of() makes a
frame with exactly that histogram.  Every family is a function of N (the pixels of the frame), so one family serves the
64x64 context (one histogram workgroup), 256x257 (several workgroups flushing into one histogram), the tiny contexts where
N * p // 10000 == 0, and the f*W x f*H sources of nmi_reduce_frame.  Each case carries the premises it was built to force --
("c", e, x): the running sum c[e] == x; ("pair", lo, hi); ("extent", vmin, vmax); ("den", T - c0); ("cc", v, c'[v] - c0);
("first", relation of h[vmin] to the plateau) -- which tests/test_tone_cases_plan.py checks on the CPU from the histogram alone.
reach() states, again from the histogram alone, on which side of each comparison of the table scan a case sits.
"""
import fractions
import functools

import numpy as np

from helpers import tone_np as tnp

LEVELS = tnp.LEVELS
SEG = 1024                      # levels of a table workgroup's segment
WAVE = 256                      # levels of a wave within it (64 lanes x 4 levels)
SHARES = [(0, 0), (1, 0), (0, 1), (100, 100), (250, 100), (2500, 2500), (5000, 4999), (9999, 0), (0, 9999)]
SHARES_FEW = [(1, 0), (250, 100), (5000, 4999), (0, 9999)]
BITS = [8, 10, 12, 14, 15, 16]
# (den, cc) = (T - c0, c'[v] - c0) whose quotient is an exact half: rounds up by the header's rule
HALVES = [(2, 1), (6, 3), (10, 1), (98, 49), (196, 98)]
# pairs named in the issue whose truncated fp64 product lies below the true floor (test_tone_cases_plan.py recomputes all)
NAMED_LOW = [(98, 49), (103, 41), (196, 98), (374, 11)]


class Case:
    def __init__(self, family, name, raw, bits, tm, premises, frame=None):
        self.family, self.name, self.bits, self.tm, self.premises = family, name, bits, tm, list(premises)
        self.raw = {int(v): int(c) for v, c in raw.items() if c}
        assert all(0 <= v < LEVELS and c > 0 for v, c in self.raw.items()), (name, raw)
        self.n = sum(self.raw.values())
        self._frame = frame     # explicit pixels (the quarter family's row patterns); else frame_of(raw)

    @property
    def m(self):
        return (1 << self.bits) - 1

    def hist(self):
        """int64 [65536]: the counts of v = min(raw, M)."""
        h = np.zeros(LEVELS, np.int64)
        for v, c in self.raw.items():
            h[min(v, self.m)] += c
        return h

    def frame(self, w, h_rows, seed=0):
        if self._frame is not None:
            assert self._frame.shape == (h_rows, w), (self.name, self._frame.shape)
            return self._frame
        return frame_of(self.raw, w, h_rows, seed)

    def twin(self):
        """(table uint8 [65536], (lo, hi)) by tests/helpers/tone_np.py."""
        return tnp.table(self.tm, self.hist())

    def __repr__(self):
        return f"{self.family}:{self.name}"


def dense(h):
    if isinstance(h, dict):
        out = np.zeros(LEVELS, np.int64)
        for v, c in h.items():
            out[v] += c
        return out
    return np.asarray(h, np.int64)


def frame_of(h, w, h_rows, seed=0):
    """A uint16 [h_rows, w] frame whose histogram of raw values is exactly h (counts [65536], or a sparse {value: count})."""
    h = dense(h)
    assert h.shape == (LEVELS,) and (h >= 0).all() and int(h.sum()) == w * h_rows, (int(h.sum()), w, h_rows)
    px = np.repeat(np.arange(LEVELS, dtype=np.uint16), h)
    np.random.default_rng(seed).shuffle(px)
    return px.reshape(h_rows, w)


def add(raw, v, c):
    if c:
        raw[v] = raw.get(v, 0) + c


def ranks(n, p_lo, p_hi):
    """(k_lo, rank_hi): lo = the smallest v with c[v] > k_lo, hi = the smallest v with c[v] >= rank_hi."""
    return n * p_lo // 10000, n - n * p_hi // 10000


# --- rank on an edge -----------------------------------------------------------------------------------------------------------

def edge_levels(bits):
    """Levels at lane (3/4), wave (255/256) and segment edges (1023/1024, a middle and the last segment's), and the range's ends."""
    m = (1 << bits) - 1
    segs = (m + 1 + SEG - 1) // SEG
    out = {3, 4, 255, 256, 0, m - 1, m}
    for k in {1, segs // 2, segs - 1}:
        if k >= 1:
            out |= {SEG * k - 1, SEG * k}
    return sorted(v for v in out if 0 <= v <= m)


def plant_running_sum(e, x, n, m):
    """A sparse histogram of n pixels with c[e] == x: x pixels at or below e (one of them on e), n - x above it (one of them on
    e + 1, the others 1500 levels up or at raw 65535, which saturates when M < 65535).  None where that cannot be."""
    if not 0 <= x <= n or (e >= m and x != n):
        return None
    raw = {}
    if x:
        add(raw, e, 1 if e > 0 and x > 1 else x)
        if e > 0 and x > 1:
            add(raw, e // 2, x - 1)
    if n - x:
        add(raw, e + 1, 1)
        add(raw, e + 1 if e + 1 == LEVELS - 1 else min(e + 1500, LEVELS - 1), n - x - 1)
    return raw


def rank_edge(n, bits=16, shares=SHARES, edges=None):
    """c[e] == k_lo + d, and separately c[e] == rank_hi + d, for d in -1, 0, +1 at every edge level e and pair of shares."""
    m = (1 << bits) - 1
    out = []
    for p_lo, p_hi in shares:
        k_lo, rank_hi = ranks(n, p_lo, p_hi)
        tm = tnp.tone(tnp.PERCENTILE, bits, p_lo=p_lo, p_hi=p_hi)
        for e in edges or edge_levels(bits):
            for side, k in (("k_lo", k_lo), ("rank_hi", rank_hi)):
                for d in (-1, 0, 1):
                    raw = plant_running_sum(e, k + d, n, m)
                    if raw is not None:
                        out.append(Case("rank", f"p{p_lo}-{p_hi}/c[{e}]=={side}{d:+d}/b{bits}/n{n}", raw, bits, tm, [("c", e, k + d)]))
    return out


# lo and hi in one lane's quad, one wave, one segment, adjacent segments, the first and the last segment (empty segments between
# the occupied ones), and far above an empty foot (segments 0 .. 38 empty)
PLACES = [(4000, 4003), (4104, 4296), (5130, 6020), (2047, 2048), (2040, 3000), (5, 65000), (40000, 40001), (1, 65534), (64512, 65535)]


def rank_places(n, bits=16, shares=((100, 100), (2500, 2500), (250, 100))):
    """c[a - 1] == k_lo and c[b] == rank_hi with lo == a and hi == b at the PLACES; and lo == hi == a reached with nonzero shares."""
    m = (1 << bits) - 1
    out = []
    for p_lo, p_hi in shares:
        k_lo, rank_hi = ranks(n, p_lo, p_hi)
        tm = tnp.tone(tnp.PERCENTILE, bits, p_lo=p_lo, p_hi=p_hi)
        if k_lo < 1 or rank_hi - k_lo < 2 or n - rank_hi < 1:
            continue
        for a, b in PLACES:
            if b + 1 > m:
                continue
            raw = {}
            add(raw, a - 1, k_lo)
            add(raw, a, 1)
            add(raw, b, rank_hi - k_lo - 1)
            add(raw, b + 1, n - rank_hi)
            out.append(Case("rank", f"p{p_lo}-{p_hi}/lo{a}-hi{b}/b{bits}/n{n}", raw, bits, tm,
                            [("c", a - 1, k_lo), ("c", b, rank_hi), ("pair", a, b), ("segments", sorted({v // SEG for v in (a - 1, a, b, b + 1)}))]))
            raw = {}
            add(raw, a - 1, k_lo)
            add(raw, a, rank_hi - k_lo)
            add(raw, a + 1, n - rank_hi)
            out.append(Case("rank", f"p{p_lo}-{p_hi}/lo==hi=={a}/b{bits}/n{n}", raw, bits, tm,
                            [("c", a - 1, k_lo), ("c", a, rank_hi), ("pair", a, a)]))
    return out


def rank_tiny(n):
    """Frames of a few pixels (N * p // 10000 == 0 for the small shares; n == 1: one pixel is the whole statistic)."""
    out = []
    if n == 1:
        for bits, v in ((16, 0), (16, 1023), (16, 1024), (16, 65535), (12, 4095), (12, 65535), (15, 40000)):
            for p_lo, p_hi in SHARES:
                tm = tnp.tone(tnp.PERCENTILE, bits, p_lo=p_lo, p_hi=p_hi)
                vs = min(v, (1 << bits) - 1)
                out.append(Case("rank", f"p{p_lo}-{p_hi}/one-pixel-{v}/b{bits}", {v: 1}, bits, tm, [("pair", vs, vs)]))
        return out
    return rank_edge(n, 16, SHARES, [0, 1023, 1024, 65534]) + rank_edge(n, 12, SHARES_FEW, [1023, 4094, 4095])


# --- extent ----------------------------------------------------------------------------------------------------------------------

def extent(n, bits_list=BITS):
    """EQUALIZE with vmin and vmax at 0, 1023, 1024, M - 1, M: one occupied level (T == c0), two, three; and raw values above M."""
    out = []
    for bits in bits_list:
        m = (1 << bits) - 1
        tm = tnp.tone(tnp.EQUALIZE, bits)
        at = sorted({v for v in (0, 1023, 1024, m - 1, m) if v <= m})
        for vmin in at:
            out.append(Case("extent", f"one-{vmin}/b{bits}/n{n}", {vmin: n}, bits, tm, [("extent", vmin, vmin), ("den", 0)]))
            for vmax in at:
                if vmax <= vmin or n < 2:
                    continue
                a = max(n // 3, 1)
                out.append(Case("extent", f"two-{vmin}-{vmax}/b{bits}/n{n}", {vmin: a, vmax: n - a}, bits, tm,
                                [("extent", vmin, vmax), ("den", n - a)]))
                mid = (vmin + vmax) // 2
                if vmin < mid < vmax and n >= 4:
                    out.append(Case("extent", f"three-{vmin}-{mid}-{vmax}/b{bits}/n{n}", {vmin: 1, mid: n // 2, vmax: n - 1 - n // 2}, bits, tm,
                                    [("extent", vmin, vmax), ("den", n - 1)]))
        if bits < 16 and n >= 8:   # h[M] collects the saturated pixels, and the entries above M equal entry M
            for vmin in (0, m - 1, m):
                raw = {}
                add(raw, vmin, n // 4)
                add(raw, m, 1)
                add(raw, m + 1, n // 4)
                add(raw, m + 1000, n // 8)
                add(raw, LEVELS - 1, n - n // 4 - 1 - n // 4 - n // 8)
                out.append(Case("extent", f"saturated-{vmin}/b{bits}/n{n}", raw, bits, tm,
                                [("extent", vmin, m), ("hM", n - (n // 4 if vmin < m else 0))]))
    return out


# --- plateau -----------------------------------------------------------------------------------------------------------------------

PLATEAU_LEVELS = [700, 1023, 1024, 5000, 5003, 30000, 65535]


def plateau(n, bits=16):
    """Distinct counts over levels in several lanes, waves and segments; the plateau at 1, the smallest count (+1), the largest
    (-1, +1).  The first occupied level holds a middle count (clipped by the small plateaus, not by the large ones), the smallest
    (never above a plateau) or the largest."""
    if n < 200:
        return []
    m = (1 << bits) - 1
    levels = sorted({min(v, m) for v in PLATEAU_LEVELS})
    base = [12, 3, 7, 20, 31, 5][:len(levels) - 1]
    counts = base + [n - sum(base)]
    small, large = min(counts), max(counts)
    assert len(set(counts)) == len(counts) and small > 1 and large == counts[-1]
    out = []
    for first in ("middle", "smallest", "largest"):
        c = list(counts)
        i = {"middle": 0, "smallest": c.index(small), "largest": len(c) - 1}[first]
        c[0], c[i] = c[i], c[0]
        raw = dict(zip(levels, c))
        for p in (1, small, small + 1, large - 1, large, large + 1):
            rel = "above" if c[0] > p else "equal" if c[0] == p else "below"
            clipped = sum(x > p for x in c)
            out.append(Case("plateau", f"first-{first}/plateau{p}/b{bits}/n{n}", raw, bits, tnp.tone(tnp.EQUALIZE, bits, plateau=p),
                            [("first", rel), ("clipped", clipped), ("extent", levels[0], levels[-1])]))
    return out


# --- quotient ------------------------------------------------------------------------------------------------------------------------

def truncated(num, den):
    """The kernel's first guess at floor(num / den): the fp64 product with the rounded reciprocal, truncated."""
    return (np.asarray(num, np.float64) * (1.0 / np.float64(den))).astype(np.int64)


@functools.lru_cache(maxsize=None)
def product_misses(limit=3000):
    """-> (below, above): the (den, cc) with den < limit, 0 <= cc <= den whose truncated product for num = cc * 255 + den // 2
    lies below / above floor(num / den)."""
    below, above = [], []
    for den in range(1, limit):
        cc = np.arange(den + 1, dtype=np.int64)
        num = cc * 255 + den // 2
        q, f = truncated(num, den), num // den
        below += [(den, int(c)) for c in cc[q < f]]
        above += [(den, int(c)) for c in cc[q > f]]
    return below, above


def quotient_histogram(n, den, ccs, bits=16, start=900, step=341):
    """h with T - c0 == den and c'[v] - c0 == cc at successive levels (start + step, start + 2 step, ...) for each cc; the first
    level `start` holds the other n - den pixels."""
    ccs = sorted(set(c for c in ccs if 0 < c <= den))
    assert 0 < den < n
    raw, prem, run = {start: n - den}, [("den", den)], 0
    v = start
    for cc in ccs:
        v += step
        add(raw, v, cc - run)
        run = cc
        prem.append(("cc", v, cc))
    if den - run:
        add(raw, v + step, den - run)
    return raw, prem


def quotient(n, bits=16, most=24):
    """Exact halves, and quotients whose truncated fp64 product is one below the floor (floor_div's ++q line): the named pairs, and
    the `most` denominators below n with the most such cc, all of them planted in one histogram each."""
    out = []
    tm = tnp.tone(tnp.EQUALIZE, bits)
    for den, cc in HALVES:
        if den < n:
            raw, prem = quotient_histogram(n, den, [cc], bits)
            out.append(Case("quotient", f"half-{den}-{cc}/n{n}", raw, bits, tm, prem + [("half", den, cc)]))
    below, _ = product_misses()
    by_den = {}
    for den, cc in below:
        by_den.setdefault(den, []).append(cc)
    chosen = sorted(by_den, key=lambda d: (-len(by_den[d]), d))[:most]
    for den in sorted(set(chosen) | {d for d, _ in NAMED_LOW}):
        if den < n:
            raw, prem = quotient_histogram(n, den, by_den[den][:60], bits, step=17)
            out.append(Case("quotient", f"low-{den}x{len(by_den[den][:60])}/n{n}", raw, bits, tm, prem + [("low", den, c) for c in by_den[den][:60]]))
    return out


# --- quarters (the histogram kernel's passes) ----------------------------------------------------------------------------------------

QUARTER_EDGES = [16383, 16384, 32767, 32768, 49151, 49152, 65535]


def quarter_tones(bits):
    return [("eq", tnp.tone(tnp.EQUALIZE, bits)), ("pct", tnp.tone(tnp.PERCENTILE, bits, p_lo=100, p_hi=100))]


def quarters(n, w=None, h_rows=None):
    """Values only at the quarter edges; every pixel in one upper quarter (at 15 bits quarters 2 and 3 saturate into quarter 1's
    32767); with a shape: rows that alternate between two quarters."""
    out = []
    for bits in (15, 16):
        for tag, tm in quarter_tones(bits):
            if n >= 2 * len(QUARTER_EDGES):
                raw = {v: n // 7 + k for k, v in enumerate(QUARTER_EDGES[:-1])}
                raw[65535] = n - sum(raw.values())
                out.append(Case("quarters", f"edges/{tag}/b{bits}/n{n}", raw, bits, tm, [("quarters", (1 << (1 << (bits - 14))) - 1)]))
            for q in (1, 2, 3):
                lo = q * 16384
                raw = {lo: max(n // 5, 1)}
                add(raw, lo + 9000, n // 3)
                add(raw, lo + 16383, n - sum(raw.values()))
                qs = 1 << (min(q, 1) if bits == 15 else q)
                out.append(Case("quarters", f"all-in-{q}/{tag}/b{bits}/n{n}", raw, bits, tm, [("quarters", qs)]))
            if w is not None:
                for qa, qb in ((0, 3), (1, 2), (3, 1)):
                    rng = np.random.default_rng(qa * 4 + qb)
                    px = np.empty((h_rows, w), np.uint16)
                    for y in range(h_rows):
                        q = qa if y % 2 == 0 else qb
                        px[y] = q * 16384 + rng.choice([0, 1, 8191, 16382, 16383], size=w)
                    raw = dict(zip(*np.unique(px, return_counts=True)))
                    out.append(Case("quarters", f"rows-{qa}-{qb}/{tag}/b{bits}/{w}x{h_rows}", raw, bits, tm, [("rows", qa, qb)], frame=px))
    return out


def quarters_planted(n):
    """One value 65,535 / 65,536 / 65,537 times in each upper quarter (n > 65,537), the other pixels spread over 300 other values."""
    out = []
    for value in (20000, 40000, 60000):
        for count in (65535, 65536, 65537):
            rest = n - count
            assert rest > 0
            rng = np.random.default_rng(value + count)
            others = rng.choice(65535, size=300, replace=False)
            others[others >= value] += 1
            raw = {int(v): int(c) for v, c in zip(*np.unique(rng.choice(others, size=rest), return_counts=True))}
            raw[value] = count
            tm = tnp.tone(tnp.EQUALIZE, 16) if count != 65536 else tnp.tone(tnp.PERCENTILE, 16, p_lo=100, p_hi=100)
            out.append(Case("quarters", f"planted-{value}x{count}/n{n}", raw, 16, tm, [("h", value, count)]))
    return out


# --- the case table --------------------------------------------------------------------------------------------------------------

SMALL, BIG = (64, 64), (256, 257)       # N = 4,096: one histogram workgroup; N = 65,792: 17 of them
TINY = [(1, 1), (5, 3)]
ROWS = [(7, 16), (8, 16), (9, 16)]      # ragged last run of a row, whole runs, one pixel over


@functools.lru_cache(maxsize=None)
def groups():
    """{group name: ((w, h), [cases])}: one GPU test function's work each, on one context."""
    n, nb = SMALL[0] * SMALL[1], BIG[0] * BIG[1]
    g = {}
    for p in SHARES:
        g[f"rank-p{p[0]}-{p[1]}"] = (SMALL, rank_edge(n, 16, [p]))
    g["rank-places"] = (SMALL, rank_places(n))
    g["rank-12-bits"] = (SMALL, rank_edge(n, 12, SHARES_FEW[1:3]))       # levels above M, raw values above M
    g["rank-15-bits"] = (SMALL, rank_edge(n, 15, SHARES_FEW[1:], [16383, 16384, 32766, 32767]))
    for w, h in TINY:
        g[f"rank-{w}x{h}"] = ((w, h), rank_tiny(w * h))
    g["extent"] = (SMALL, extent(n))
    g["extent-1x1"] = ((1, 1), extent(1, [8, 12, 16]))
    g["plateau"] = (SMALL, plateau(n) + plateau(n, 12))
    g["quotient"] = (SMALL, quotient(n))
    g["quarters"] = (SMALL, quarters(n))
    for w, h in ROWS:
        g[f"quarters-{w}x{h}"] = ((w, h), quarters(w * h, w, h))
    for p in SHARES_FEW:
        g[f"big-rank-p{p[0]}-{p[1]}"] = (BIG, rank_edge(nb, 16, [p]))
    g["big-rank-places"] = (BIG, rank_places(nb))
    g["big-extent"] = (BIG, extent(nb, [8, 12, 15, 16]))
    g["big-plateau"] = (BIG, plateau(nb))
    g["big-quotient"] = (BIG, quotient(nb, most=8))
    g["big-quarters"] = (BIG, quarters(nb) + quarters_planted(nb))
    return g


def family_counts():
    out = {}
    for _, cases in groups().values():
        for c in cases:
            out[c.family] = out.get(c.family, 0) + 1
    return out


def one_per_family(n):
    """A case of each family for a frame of n pixels, and a partner whose lo / hi (or extent) lie in other segments: what a level
    or a stream alternates between."""
    k = lambda cases, part: next(c for c in cases if part in c.name)
    return [(k(rank_places(n), "lo4104-hi4296"), k(rank_places(n), "lo5-hi65000")),
            (k(rank_edge(n, 16, [(250, 100)]), "c[1023]==k_lo+0"), k(rank_edge(n, 16, [(250, 100)]), "c[32768]==rank_hi+0")),
            (k(extent(n, [14]), "three-0-"), k(extent(n, [14]), "saturated-16382")),
            (k(plateau(n), "first-middle/plateau4"), k(plateau(n, 12), "first-largest/plateau3")),
            (k(quotient(n), "low-98x"), k(quotient(n), "half-10-1")),
            (k(quarters(n), "all-in-2/eq/b15"), k(quarters(n), "edges/pct/b16"))]


# --- the rule, stated independently of the twin ----------------------------------------------------------------------------------

def half_up(q):
    """A Fraction rounded to the nearest integer, halves up."""
    return (q + fractions.Fraction(1, 2)).__floor__()


def exact_rule(case, h, pair):
    """-> f(v): entry v of the table by the header's rule in exact rationals, given the histogram and the {lo, hi} pair."""
    tm, m = case.tm, case.m
    lo, hi = pair
    if tm["mode"] == tnp.PERCENTILE:
        def window(v):
            v = min(v, m)
            return 0 if v <= lo else 255 if v >= hi else half_up(fractions.Fraction((v - lo) * 255, hi - lo))
        return window
    at = [int(x) for x in np.flatnonzero(h)]
    hc = [min(int(h[a]), tm["plateau"]) if tm["plateau"] else int(h[a]) for a in at]
    t, c0 = sum(hc), hc[0]

    def equalize(v):
        v = min(v, m)
        if t == c0 or v < at[0]:
            return 0
        return half_up(fractions.Fraction((sum(c for a, c in zip(at, hc) if a <= v) - c0) * 255, t - c0))
    return equalize


def exact_pair(case, px):
    """(lo, hi) from the pixels themselves: order statistics for PERCENTILE, the extent for EQUALIZE."""
    s = np.sort(np.minimum(np.asarray(px, np.int64), case.m).ravel())
    if case.tm["mode"] == tnp.PERCENTILE:
        n = s.size
        k_lo, k_hi = n * case.tm["p_lo"] // 10000, n * case.tm["p_hi"] // 10000
        return int(s[k_lo]), int(s[n - k_hi - 1])
    return int(s[0]), int(s[-1])


def check_table_exactly(case, lut, pair):
    """The table is non-decreasing and equals the exact rule on both sides of each of its steps and at its ends.  The rule is
    non-decreasing too, so a table that passes equals it at all 65,536 entries (between two checked points of equal value
    neither can move)."""
    t = lut.astype(np.int64)
    assert (np.diff(t) >= 0).all(), case
    steps = np.flatnonzero(np.diff(t))
    rule = exact_rule(case, case.hist(), pair)
    for v in sorted({0, LEVELS - 1, *steps.tolist(), *(steps + 1).tolist()}):
        assert t[v] == rule(v), (case, v, int(t[v]))
    return len(steps)


# --- which side of each comparison a case sits on --------------------------------------------------------------------------------

def sign(a, b):
    return "lt" if a < b else "eq" if a == b else "gt"


def reach(case):
    """The set of (comparison, side) this case decides, from its histogram alone.  A comparison is recorded where the other
    half of its conjunction holds, so that it alone decides the branch:
      seg b<=k_lo / seg e>k_lo / seg b<rank_hi / seg e>=rank_hi   over the occupied segments (b, e: running sum below, through)
      lvl before<=k_lo / lvl run>k_lo / lvl before<rank_hi / lvl run>=rank_hi   over the occupied levels of the crossing segment
      empty seg at k_lo, empty seg at rank_hi   an empty segment whose b == e equals the rank (what the seg_sum guard is about)
      wave   the wave of the crossing segment that holds the cut (w0 .. w3) with pixels in the waves below it (+) or none (-)
      record   a segment without / with pixels (the first-level record test)
      v?lo   EQUALIZE entries below, at, above vmin
      h[vmin]?plateau, T?c0, and the two correction lines of the quotient (q*den?num, (q+1)*den?num)."""
    out = set()
    h = case.hist()
    n, tm = case.n, case.tm
    seg_sum = h.reshape(-1, SEG).sum(axis=1)
    for s in range(LEVELS // SEG):
        out.add(("record", "empty" if seg_sum[s] == 0 else "occupied"))
    if tm["mode"] == tnp.PERCENTILE:
        c = np.cumsum(h)
        k_lo, rank_hi = ranks(n, tm["p_lo"], tm["p_hi"])
        seg_e = np.cumsum(seg_sum)
        seg_b = seg_e - seg_sum
        for s in range(LEVELS // SEG):
            b, e = int(seg_b[s]), int(seg_e[s])
            if seg_sum[s] == 0:
                if b == k_lo:
                    out.add(("empty seg at k_lo", "eq"))
                if b == rank_hi:
                    out.add(("empty seg at rank_hi", "eq"))
                continue
            if e > k_lo:
                out.add(("seg b<=k_lo", sign(b, k_lo)))
            if b <= k_lo:
                out.add(("seg e>k_lo", sign(e, k_lo)))
            if e >= rank_hi:
                out.add(("seg b<rank_hi", sign(b, rank_hi)))
            if b < rank_hi:
                out.add(("seg e>=rank_hi", sign(e, rank_hi)))
        lo, hi = tnp.percentile_pair(h, tm["p_lo"], tm["p_hi"])
        for cut, k, names, ok in ((lo, k_lo, ("lvl before<=k_lo", "lvl run>k_lo"), (lambda b, r: (r > k_lo, b <= k_lo))),
                                  (hi, rank_hi, ("lvl before<rank_hi", "lvl run>=rank_hi"), (lambda b, r: (r >= rank_hi, b < rank_hi)))):
            s = cut // SEG
            for v in np.flatnonzero(h[s * SEG:(s + 1) * SEG]) + s * SEG:
                run = int(c[v])
                before = run - int(h[v])
                other_for_before, other_for_run = ok(before, run)
                if other_for_before:
                    out.add((names[0], sign(before, k)))
                if other_for_run:
                    out.add((names[1], sign(run, k)))
            w = (cut % SEG) // WAVE
            out.add(("wave", f"w{w}{'+' if h[s * SEG:s * SEG + w * WAVE].sum() else '-'}"))
        out.add(("pair", sign(lo, hi)))
        return out
    at = np.flatnonzero(h)
    vmin = int(at[0])
    p = tm["plateau"]
    hc = np.minimum(h, p) if p else h
    if p:
        out.add(("h[vmin]?plateau", sign(int(h[vmin]), p)))
        out.add(("clipped", "all" if (h[at] > p).all() else "none" if (h[at] <= p).all() else "some"))
    out.add(("v?lo", "gt"))
    out.add(("v?lo", "eq"))
    if vmin > 0:
        out.add(("v?lo", "lt"))
    t, c0 = int(hc.sum()), int(hc[vmin])
    out.add(("T?c0", sign(t, c0)))
    for s in range(LEVELS // SEG):   # EQUALIZE scans every segment: levels in waves 1 .. 3 with pixels in the waves below them
        for w in range(1, SEG // WAVE):
            if seg_sum[s] and h[s * SEG + w * WAVE:s * SEG + (w + 1) * WAVE].sum():
                out.add(("wave", f"w{w}{'+' if h[s * SEG:s * SEG + w * WAVE].sum() else '-'}"))
    if t != c0:
        den = t - c0
        cc = np.cumsum(hc)[at] - c0
        num = cc * 255 + den // 2
        q = truncated(num, den)
        for qq, nn in zip(q.tolist(), num.tolist()):
            out.add(("q*den?num", sign(qq * den, nn)))
            out.add(("(q+1)*den?num", sign((qq + 1) * den, nn)))
    return out


def check_premise(case, prem):
    """True if the histogram has the property the case was built for."""
    h = case.hist()
    kind = prem[0]
    at = np.flatnonzero(h)
    p = case.tm["plateau"]
    hc = np.minimum(h, p) if p else h
    vmin = int(at[0])
    t, c0 = int(hc.sum()), int(hc[vmin])
    if kind == "c":
        return int(np.cumsum(h)[prem[1]]) == prem[2]
    if kind == "pair":
        return tnp.percentile_pair(h, case.tm["p_lo"], case.tm["p_hi"]) == (prem[1], prem[2])
    if kind == "extent":
        return (vmin, int(at[-1])) == (prem[1], prem[2])
    if kind == "den":
        return t - c0 == prem[1]
    if kind == "segments":
        return sorted(set((at // SEG).tolist())) == prem[1]
    if kind == "cc":
        return int(np.cumsum(hc)[prem[1]]) - c0 == prem[2] and h[prem[1]] > 0
    if kind == "half":
        den, cc = prem[1], prem[2]
        return den % 2 == 0 and cc * 255 % den == den // 2 and t - c0 == den and cc in (np.cumsum(hc)[at] - c0)
    if kind == "low":
        den, cc = prem[1], prem[2]
        num = cc * 255 + den // 2
        return int(truncated(num, den)) == num // den - 1 and t - c0 == den and cc in (np.cumsum(hc)[at] - c0)
    if kind == "first":
        return sign(int(h[vmin]), p) == {"above": "gt", "equal": "eq", "below": "lt"}[prem[1]]
    if kind == "clipped":
        return int((h[at] > p).sum()) == prem[1]
    if kind == "hM":
        return int(h[case.m]) == prem[1] and h[case.m + 1:].sum() == 0
    if kind == "h":
        return int(h[prem[1]]) == prem[2]
    if kind == "quarters":
        return sum(1 << q for q in set((at >> 14).tolist())) == prem[1]
    if kind == "rows":
        px = np.minimum(case._frame.astype(np.int64), case.m) >> 14
        qa, qb = (min(q, (case.m >> 14)) for q in prem[1:])
        return (px[0::2] == qa).all() and (px[1::2] == qb).all()
    raise ValueError(kind)
