"""CPU checks of the planted histograms of tests/helpers/tone_cases.py (the cases tests/test_tone_edges.py runs on the GPU):
every case has the property it was built to force; the numpy twin (tests/helpers/tone_np.py) is held to an independent statement
of the rule on every case -- order statistics of the pixels for the {lo, hi} pair, exact rationals rounded half up for every
quotient; and the case table sits on, below and above every comparison of the table scan in csrc/nmi_tone.hip."""
import numpy as np
import pytest

from helpers import tone_cases as tc
from helpers import tone_np as tnp

GROUPS = list(tc.groups())


def test_frame_of_plants_the_histogram_exactly():
    h = np.zeros(tnp.LEVELS, np.int64)
    h[[0, 3, 1023, 1024, 40000, 65535]] = [5, 1, 700, 2, 3387, 1]
    a, b = tc.frame_of(h, 64, 64, seed=1), tc.frame_of(h, 64, 64, seed=2)
    assert a.dtype == np.uint16 and a.shape == (64, 64)
    assert (tnp.histogram(a, 16) == h).all() and (tnp.histogram(b, 16) == h).all() and (a != b).any()
    assert (tc.frame_of({7: 3, 9: 12}, 5, 3) == tc.frame_of({7: 3, 9: 12}, 5, 3)).all()       # seeded
    with pytest.raises(AssertionError):
        tc.frame_of({7: 3}, 2, 2)


@pytest.mark.parametrize("group", GROUPS)
def test_every_case_has_the_property_it_was_built_for(group):
    (w, h), cases = tc.groups()[group]
    assert cases and len({c.name for c in cases}) == len(cases)
    for c in cases:
        assert c.n == w * h, c
        assert c.tm["mode"] in (tnp.PERCENTILE, tnp.EQUALIZE) and c.tm["bits"] == c.bits
        assert (tnp.histogram(c.frame(w, h), c.bits) == c.hist()).all(), c
        assert c.premises, c
        for prem in c.premises:
            assert tc.check_premise(c, prem), (c, prem)


@pytest.mark.parametrize("group", GROUPS)
def test_the_twin_equals_the_rule_stated_independently(group):
    """lo = sorted(pixels)[k_lo], hi = sorted(pixels)[N - k_hi - 1] (EQUALIZE: the smallest and the largest pixel), and the table
    in exact rationals, rounded half up, with no entry exempt."""
    (w, h), cases = tc.groups()[group]
    for c in cases:
        lut, pair = c.twin()
        assert pair == tc.exact_pair(c, c.frame(w, h)), c
        assert 0 <= pair[0] <= pair[1] <= c.m, c
        assert (lut[c.m:] == lut[c.m]).all(), c                    # the entries above M are entry M
        tc.check_table_exactly(c, lut, pair)


def test_the_truncated_product_is_never_above_the_floor():
    """The fp64 product with the rounded reciprocal, truncated, against floor(num / den) for num = cc * 255 + den // 2, all den <
    3000 and 0 <= cc <= den: 520 pairs lie one below (floor_div's ++q line makes those entries right) and none above, so the --q
    line is not reached by any case here and is not claimed as covered."""
    below, above = tc.product_misses()
    assert above == []
    assert len(below) == 520 and all(p in below for p in tc.NAMED_LOW)
    for den, cc in below:
        num = cc * 255 + den // 2
        assert int(tc.truncated(num, den)) == num // den - 1
    for den, cc in tc.HALVES:
        assert den % 2 == 0 and cc * 255 % den == den // 2
        assert tc.half_up(tc.fractions.Fraction(cc * 255, den)) == (cc * 255 + den // 2) // den == cc * 255 // den + 1


def test_the_families_are_of_the_sizes_the_suite_counts_on():
    counts = tc.family_counts()
    assert set(counts) == {"rank", "extent", "plateau", "quotient", "quarters"} and all(v >= 40 for v in counts.values()), counts
    for (w, h), cases in tc.groups().values():
        assert len(cases) <= 220, len(cases)                       # one GPU test function's work: a few seconds at most


SIDES = ("lt", "eq", "gt")
# comparison -> the sides the case table must reach.  Sides that cannot occur: T < c0 (c0 is part of T); q * den > num (the
# premise above); (q + 1) * den < num (the product is within one of the floor); lo > hi (p_lo + p_hi < 10000).
WANTED = {
    "seg b<=k_lo": SIDES, "seg e>k_lo": SIDES, "seg b<rank_hi": SIDES, "seg e>=rank_hi": SIDES,
    "lvl before<=k_lo": SIDES, "lvl run>k_lo": SIDES, "lvl before<rank_hi": SIDES, "lvl run>=rank_hi": SIDES,
    "empty seg at k_lo": ("eq",), "empty seg at rank_hi": ("eq",),
    "wave": ("w0-", "w1-", "w1+", "w2+", "w3+"),
    "record": ("empty", "occupied"),
    "pair": ("lt", "eq"),
    "v?lo": SIDES,
    "h[vmin]?plateau": SIDES,
    "clipped": ("all", "some", "none"),
    "T?c0": ("eq", "gt"),
    "q*den?num": ("lt", "eq"),
    "(q+1)*den?num": ("eq", "gt"),
}


def test_the_case_table_sits_on_every_comparison_of_the_scan():
    """For each comparison of nmi_tone_table_kernel and nmi_tone_sums_kernel: a case with equality and one on each side, found
    from the histograms alone.  Per shape too: the 64x64 and the 256x257 groups each reach all of it."""
    for prefix in ("", "big-"):
        reached = {}
        for name, (_, cases) in tc.groups().items():
            if name.startswith("big-") != (prefix == "big-"):
                continue
            for c in cases:
                for comparison, side in tc.reach(c):
                    reached.setdefault(comparison, set()).add(side)
        for comparison, sides in WANTED.items():
            missing = set(sides) - reached.get(comparison, set())
            assert not missing, (prefix, comparison, missing)
        assert "lt" not in reached["T?c0"] and "gt" not in reached["q*den?num"] and "gt" not in reached["pair"]
        assert "lt" not in reached["(q+1)*den?num"]


def test_the_pipeline_subset_alternates_frames_of_other_segments():
    for n in (64 * 48, 4 * 4096, 9 * 4096):
        pairs = tc.one_per_family(n)
        assert [a.family for a, _ in pairs] == ["rank", "rank", "extent", "plateau", "quotient", "quarters"]
        for a, b in pairs:
            assert a.n == b.n == n and a.family == b.family
            (_, pa), (_, pb) = a.twin(), b.twin()
            assert pa != pb and (pa[0] // tc.SEG, pa[1] // tc.SEG) != (pb[0] // tc.SEG, pb[1] // tc.SEG), (a, b, pa, pb)
