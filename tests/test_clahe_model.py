"""CPU tests of the CLAHE model (tests/helpers/clahe_np.py), the premises of the GPU tests of tests/test_clahe_*.py: the
vectorised model equals the naive restatement, the rule's invariants hold, and the planted cases of tests/helpers/clahe_cases.py
hit the boundaries they name."""
import numpy as np
import pytest

from helpers import clahe_cases as cases
from helpers import clahe_np as cnp
from helpers import tone_np as tnp


@pytest.mark.parametrize("w,h,tx,ty,bits,plateau", [
    (64, 48, 8, 8, 10, 0), (64, 48, 8, 8, 10, 2), (70, 50, 8, 8, 10, 1), (64, 48, 3, 2, 8, 3), (64, 48, 1, 1, 8, 7),
    (8, 6, 8, 6, 8, 1), (20, 14, 2, 2, 16, 1), (9, 70, 8, 3, 12, 0),
])
def test_the_vectorised_model_equals_the_naive_form(w, h, tx, ty, bits, plateau):
    rng = np.random.default_rng(w + tx + bits)
    px = np.where(rng.random((h, w)) < 0.5, rng.integers(0, 65536, (h, w)), rng.integers(100, 140, (h, w))).astype(np.uint16)
    tm = cnp.clahe(tx, ty, plateau, bits)
    want, tables, counts = cnp.naive_apply(px, tm)
    luts, n = cnp.tile_luts(px, tm)
    L = 1 << bits
    assert (n == np.array(counts)).all()
    assert (luts[:, :, :L] == np.array(tables, np.uint8)).all()
    assert (luts[:, :, L:] == luts[:, :, L - 1:L]).all()
    assert (cnp.apply(px, tm) == want).all()


@pytest.mark.parametrize("bits", [8, 10, 16])
@pytest.mark.parametrize("n,plateau", [(48, 1), (504, 1), (504, 3), (3072, 1), (3072, 100), (70000, 1), (70000, 5)])
def test_the_closed_form_is_the_loop_and_ends_at_the_pixel_count(bits, n, plateau):
    rng = np.random.default_rng(n + bits)
    m = (1 << bits) - 1
    values = np.minimum(np.where(rng.random(n) < 0.6, 77, rng.integers(0, 65536, n)), m)
    h = np.bincount(values, minlength=cnp.LEVELS)[None, :]
    t, count = cnp.tables_of_histograms(h, bits, plateau)
    c2 = cnp.running(h, plateau, bits)
    assert count[0] == n and c2[0, m] == n and t.max() <= 255
    if bits <= 10:
        assert (t[0, :m + 1] == np.array(cnp.naive_table(list(values), bits, plateau), np.uint8)).all()


@pytest.mark.parametrize("size,tiles", sorted(cases.AXES))
def test_no_tile_is_empty_and_the_edges_are_where_the_rule_puts_them(size, tiles):
    t = cnp.tile_of(size, tiles)
    assert (np.bincount(t, minlength=tiles) > 0).all() and t.max() == tiles - 1 and (np.diff(t) >= 0).all()
    lo, hi, w = cnp.axis(size, tiles)
    # the first and last half tile: clamped neighbours (a one-pixel tile's centre is the pixel: the neighbour weighs 0)
    assert lo[0] == 0 and (hi[0] == 0 or w[0] == 0) and lo[-1] == hi[-1] == tiles - 1
    if size >= 2 * tiles:
        assert hi[0] == 0 and cnp.axis(size, tiles)[0][size // (2 * tiles) - 1] == 0
    if tiles > 1:
        assert (hi - lo).max() == 1


def test_every_axis_the_gpu_tests_use_is_listed():
    for w, h, tx, ty in cases.GRIDS.values():
        assert (w, tx) in cases.AXES and (h, ty) in cases.AXES
    for f in cases.FACTORS:
        w, h, tx, ty = cases.REDUCED
        assert (f * w, tx) in cases.AXES and (f * h, ty) in cases.AXES


@pytest.mark.parametrize("plateau", [0, 1, 4])
def test_equal_tile_histograms_give_the_single_table_result(plateau):
    """A frame of identical tiles: every pixel is its tile's table value, whatever the weights."""
    rng = np.random.default_rng(5)
    cell = rng.integers(0, 1024, (6, 8)).astype(np.uint16)
    px = np.tile(cell, (8, 8))                                             # 64 x 48 in 8 x 8 tiles of 8 x 6
    tm = cnp.clahe(8, 8, plateau, 10)
    luts, n = cnp.tile_luts(px, tm)
    assert (n == 48).all() and (luts == luts[0, 0]).all()
    assert (cnp.apply(px, tm) == luts[0, 0][px]).all()
    if plateau == 0:    # 64 times the counts over 64 times the pixels: the whole frame's one table is the tile's
        assert (cnp.apply(px, tm) == cnp.apply(px, cnp.clahe(1, 1, 0, 10))).all()


@pytest.mark.parametrize("name", list(cases.PLANTED))
def test_the_planted_cases_hit_their_boundaries(name):
    case = cases.PLANTED[name]
    px, tm = cases.planted(name)
    w, h, tx, ty = cases.GRIDS[case["grid"]]
    hist = cnp.tile_histograms(px, tm["bits"], tx, ty)[0]                  # the planted tile is tile (0, 0)
    e, q, r, step = cnp.excess(hist, tm["plateau"], tm["bits"])
    L = 1 << tm["bits"]
    want = case["expect"]
    got = {"E": e, "q": q, "r": r, "step": step, "L": L, "n": int(hist.sum()), "top": int(hist.max())}
    for key, value in want.items():
        assert got[key] == value, (name, key, got)


def test_the_contents_are_what_the_gpu_tests_say_they_are():
    assert tnp.histogram(cases.content("uniform", 70, 50, 16), 16).max() == 1  # every bin <= 1
    px = cases.content("over_depth", 64, 48, 12)
    assert (px > 4095).any() and cnp.tile_histograms(px, 12, 8, 8)[:, 4095].min() > 0     # saturation reaches every tile
    left_right = cnp.halves(64, 48)
    luts, _ = cnp.tile_luts(left_right, cnp.clahe(8, 8, 0, 16))
    assert (luts[0, 0] != luts[0, 7]).any()
    out = cnp.apply(left_right, cnp.clahe(8, 8, 0, 16))
    single = cnp.apply(left_right, cnp.clahe(1, 1, 0, 16))
    assert (out != single).any()                                          # the blend is not hidden by equal tables
