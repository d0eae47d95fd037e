"""CPU checks of the numpy twin of the full-size frame reduction (tests/helpers/reduce_np.py; nmi_reduce_frame, include/nmi_hip.h):
the integer rounding rules against the float32 form they restate and against the exact mean, for every possible sum; the twin on
colour frames; the mask rule."""
import numpy as np
import pytest

from helpers import color_np as cnp
from helpers import reduce_np as rnp


@pytest.mark.parametrize("f", [2, 3, 4])
def test_integer_rule_for_every_sum(f):
    s = np.arange(255 * f * f + 1)
    got = rnp.round_sum(s, f).astype(np.int64)
    assert (got == rnp.float_form(s, f)).all(), s[got != rnp.float_form(s, f)][:8]
    mean = s.astype(np.float64) / (f * f)
    assert (np.abs(got - mean) <= 0.5).all()
    g = np.arange(256)
    assert (rnp.round_sum(g * f * f, f) == g).all()      # a constant frame g -> g


def test_factor_one_is_the_identity():
    s = np.arange(256)
    assert (rnp.round_sum(s, 1) == s).all()
    g = np.random.default_rng(1).integers(0, 256, (6, 8), dtype=np.uint8)
    assert (rnp.reduce_gray(g, 1) == g).all()


def test_four_rounds_halves_to_even_and_two_rounds_them_up():
    assert rnp.round_sum([8, 24, 40, 56], 4).tolist() == [0, 2, 2, 4]       # 0.5, 1.5, 2.5, 3.5
    assert rnp.round_sum([2, 6, 10], 2).tolist() == [1, 2, 3]              # 0.5, 1.5, 2.5: the 2x2 path's (s + 2) >> 2
    assert np.rint(np.array([2, 6, 10]) / 4).tolist() == [0, 2, 2]         # where rint would differ: f = 2 is not that form


@pytest.mark.parametrize("f", [2, 3, 4])
def test_hand_made_blocks(f):
    g = np.zeros((2 * f, 3 * f), np.uint8)
    g[:f, :f] = 200
    g[:f, f:2 * f] = np.arange(f * f).reshape(f, f)
    g[f:, 2 * f:] = 255
    g[f, 0] = 255                                       # one bright pixel in a dark block
    want = np.array([[200, rnp.round_sum(sum(range(f * f)), f), 0], [rnp.round_sum(255, f), 0, 255]], np.uint8)
    assert (rnp.reduce_gray(g, f) == want).all()


@pytest.mark.parametrize("fmt", cnp.COLOR_FORMATS, ids=["bgr", "rgb", "bgra", "rgba"])
@pytest.mark.parametrize("f", [1, 2, 3, 4])
def test_colour_is_to_gray_then_the_grey_reduction(f, fmt):
    w, h = 7, 5
    rng = np.random.default_rng(f * 5 + fmt)
    rgb = rng.integers(0, 256, (h * f, w * f, 3), dtype=np.uint8)
    for pitch, off in [(0, 0), (w * f * cnp.BPP[fmt] + 5, 3)]:
        buf = cnp.pack(rgb, fmt, pitch, off, seed=f)
        gray = cnp.to_gray(buf, fmt, w * f, h * f, pitch, off)
        assert (gray == cnp.gray_of(rgb[..., 0], rgb[..., 1], rgb[..., 2])).all()
        got = rnp.reduce_frame(buf, fmt, w, h, f, pitch, off)
        assert got.shape == (h, w) and got.dtype == np.uint8
        assert (got == rnp.reduce_gray(gray, f)).all()
        # pixel by pixel, from the definition
        for y, x in [(0, 0), (h - 1, w - 1), (2, 3)]:
            s = int(gray[f * y:f * y + f, f * x:f * x + f].astype(np.int64).sum())
            assert got[y, x] == rnp.round_sum(s, f)


def test_a_wider_pitch_crops_spare_columns_and_rows():
    """1241x376 at f = 2 gives 620x188: the last source column is never read."""
    rng = np.random.default_rng(2)
    g = rng.integers(0, 256, (376, 1241), dtype=np.uint8)
    buf = cnp.pack(g, cnp.GRAY)
    a = rnp.reduce_frame(buf, cnp.GRAY, 620, 188, 2, pitch=1241)
    g2 = g.copy()
    g2[:, 1240] ^= 0xFF
    b = rnp.reduce_frame(cnp.pack(g2, cnp.GRAY), cnp.GRAY, 620, 188, 2, pitch=1241)
    assert a.shape == (188, 620) and (a == b).all()
    assert (a == rnp.reduce_gray(g[:, :1240], 2)).all()


@pytest.mark.parametrize("f", [1, 2, 3, 4])
def test_mask_rule(f):
    m = np.ones((3 * f, 4 * f), np.uint8)
    want = np.ones((3, 4), np.uint8)
    m[0, 0] = 0                      # a corner byte of block (0, 0)
    want[0, 0] = 0
    m[2 * f - 1, 3 * f - 1] = 0      # the last byte of block (1, 2)
    want[1, 2] = 0
    m[2 * f:, f:2 * f] = 0           # all of block (2, 1)
    want[2, 1] = 0
    m[f:2 * f, 0:f] = 7              # any nonzero byte counts as set
    m[2 * f:, 3 * f:] = 255
    assert (rnp.reduce_mask(m, f) == want).all()
    assert (rnp.reduce_mask(m.astype(bool), f) == want).all()
    assert set(np.unique(rnp.reduce_mask(m, f))) <= {0, 1}


@pytest.mark.parametrize("f", [2, 3, 4])
def test_every_sum_frame_holds_every_sum(f):
    g = rnp.every_sum_frame(f, 96, 48, seed=f)
    assert g.shape == (48 * f, 96 * f) and g.dtype == np.uint8
    assert len(np.unique(rnp.block_sums(g, f))) == 255 * f * f + 1
