"""CPU tests of the numpy twin of the raw sensor formats (tests/helpers/sensor_np.py; the contract is nmi_gray_frame's in
include/nmi_hip.h): the Bayer rule against its exact rational, flat and pure-channel mosaics, the four patterns, the crop
remark, reflection at (0, 0) written out by hand, and pack()'s layout."""
from fractions import Fraction

import numpy as np
import pytest

from helpers import color_np as cnp
from helpers import sensor_np as snp

BAYER = list(snp.BAYER_FORMATS.values())
BAYER_IDS = list(snp.BAYER_FORMATS)


def exact(r4, g4, b4):
    return Fraction(4899 * int(r4) + 9617 * int(g4) + 1868 * int(b4), 65536)


@pytest.mark.parametrize("fmt", BAYER, ids=BAYER_IDS)
def test_twin_is_within_half_of_the_exact_rational(fmt):
    rng = np.random.default_rng(fmt)
    for w, h in ((2, 2), (3, 2), (5, 3), (17, 12)):
        m = rng.integers(0, 256, (h, w), dtype=np.uint8)
        m[rng.random((h, w)) < 0.2] = 255         # saturated neighbourhoods too
        r4, g4, b4 = snp.demosaic4(m, fmt)
        got = snp.bayer_gray(m, fmt)
        for y in range(h):
            for x in range(w):
                e = exact(r4[y, x], g4[y, x], b4[y, x])
                assert abs(Fraction(int(got[y, x])) - e) <= Fraction(1, 2), (w, h, x, y)
                assert 0 <= e <= 255


@pytest.mark.parametrize("fmt", BAYER, ids=BAYER_IDS)
def test_flat_mosaic_gives_itself(fmt):
    for g in (0, 1, 127, 128, 254, 255):
        for w, h in ((2, 2), (3, 3), (8, 5)):
            assert (snp.bayer_gray(np.full((h, w), g, np.uint8), fmt) == g).all()


@pytest.mark.parametrize("fmt", BAYER, ids=BAYER_IDS)
def test_pure_channels_give_the_colour_rule_in_the_interior(fmt):
    h, w = 8, 10
    for v in (1, 77, 200, 255):
        for ch in range(3):
            rgb = np.zeros((h, w, 3), np.uint8)
            rgb[..., ch] = v
            got = snp.bayer_gray(snp.mosaic(rgb, fmt), fmt)
            want = cnp.gray_of(*(v if c == ch else 0 for c in range(3)))
            assert (got[1:-1, 1:-1] == want).all(), (v, ch)
            assert (got == want).all()            # and, reflection keeping the phase, at the edges too


def test_the_four_patterns_differ_on_a_frame_with_chroma():
    m = snp.mosaic(snp.chroma_frame(16, 12, seed=1), snp.RGGB)
    grays = [snp.bayer_gray(m, f) for f in BAYER]
    for i in range(4):
        for j in range(i + 1, 4):
            assert (grays[i] != grays[j]).any(), (i, j)


def test_a_crop_by_one_column_or_row_changes_the_pattern():
    rng = np.random.default_rng(5)
    m = rng.integers(0, 256, (13, 18), dtype=np.uint8)
    full = snp.bayer_gray(m, snp.RGGB)
    # away from the edges of either frame (reflection differs there), RGGB == GRBG one column in, GBRG one row down, BGGR both
    assert (full[1:-1, 2:-1] == snp.bayer_gray(m[:, 1:], snp.GRBG)[1:-1, 1:-1]).all()
    assert (full[2:-1, 1:-1] == snp.bayer_gray(m[1:, :], snp.GBRG)[1:-1, 1:-1]).all()
    assert (full[2:-1, 2:-1] == snp.bayer_gray(m[1:, 1:], snp.BGGR)[1:-1, 1:-1]).all()
    assert (full[1:-1, 2:-1] != snp.bayer_gray(m[:, 1:], snp.RGGB)[1:-1, 1:-1]).any()


def test_reflection_at_the_corner_by_hand():
    a, b, c, d = 200, 10, 30, 90
    m = np.array([[a, b], [c, d]], np.uint8)
    # RGGB, (0, 0) is red: p(-1, .) = p(1, .), p(., -1) = p(., 1)
    want = (4899 * 4 * a + 9617 * (b + b + c + c) + 1868 * 4 * d + 32768) >> 16
    assert snp.bayer_gray(m, snp.RGGB)[0, 0] == want
    # GRBG, (0, 0) is green in a red row: red left and right (both b), blue above and below (both c)
    want = (4899 * 2 * (b + b) + 9617 * 4 * a + 1868 * 2 * (c + c) + 32768) >> 16
    assert snp.bayer_gray(m, snp.GRBG)[0, 0] == want
    m3 = np.array([[11, 22, 33], [44, 55, 66], [77, 88, 99]], np.uint8)
    want = (4899 * 4 * 11 + 9617 * (22 + 22 + 44 + 44) + 1868 * 4 * 55 + 32768) >> 16
    assert snp.bayer_gray(m3, snp.RGGB)[0, 0] == want
    # BGGR, (2, 2) of the 3x3 is blue: W -> W - 2
    want = (4899 * 4 * 55 + 9617 * (88 + 88 + 66 + 66) + 1868 * 4 * 99 + 32768) >> 16
    assert snp.bayer_gray(m3, snp.BGGR)[2, 2] == want


def test_yuv_is_the_luma_byte_and_pack_hides_junk_everywhere_else():
    rng = np.random.default_rng(9)
    w, h = 7, 4
    img = rng.integers(0, 256, (h, w), dtype=np.uint8)
    for fmt in snp.FORMATS.values():
        bpp = snp.BPP[fmt]
        for pitch, off in ((0, 0), (w * bpp + 5, 3)):
            b1, b2 = snp.pack(img, fmt, pitch, off, seed=1), snp.pack(img, fmt, pitch, off, seed=2)
            assert len(b1) == off + snp.span(fmt, w, h, pitch)
            assert (snp.pixels(b1, fmt, w, h, pitch, off) == img).all()
            assert (snp.to_gray(b1, fmt, w, h, pitch, off) == snp.to_gray(b2, fmt, w, h, pitch, off)).all()
            if bpp == 2 or pitch or off:
                assert (b1 != b2).any()
    assert (snp.to_gray(snp.pack(img, snp.YUYV), snp.YUYV, w, h) == img).all()
    assert (snp.pack(img, snp.YUYV)[0::2] == img.reshape(-1)).all() and (snp.pack(img, snp.UYVY)[1::2] == img.reshape(-1)).all()


def test_reduce_crops_by_pitch_and_reflects_at_the_covered_edge():
    rng = np.random.default_rng(3)
    m = rng.integers(0, 256, (8, 11), dtype=np.uint8)          # 11 wide: 5 blocks of 2, the last column spare
    buf = snp.pack(m, snp.RGGB)
    got = snp.reduce_frame(buf, snp.RGGB, 5, 4, 2, pitch=11)
    want = snp.reduce_frame(snp.pack(m[:, :10].copy(), snp.RGGB), snp.RGGB, 5, 4, 2)
    assert (got == want).all()
