"""CPU tests of the valid range's numpy twin (tests/helpers/valid_np.py; the rule: include/nmi_hip.h "Deep frames"): with the range
off it is tone_np / clahe_np byte for byte; a ranged table is the table of the valid pixels' histogram alone; the N == 0 and
empty-tile rules; the mask rule at every factor; a float64 model of the quotients; and, on every planted frame the GPU tests use,
that the range changes the table and that the mask is neither all 0 nor all 1 -- so that an implementation that ignores the range
cannot pass them."""
import numpy as np
import pytest

from helpers import clahe_np as cnp
from helpers import reduce_np as rnp
from helpers import tone_np as tnp
from helpers import valid_cases as cases
from helpers import valid_np as vnp

GLOBAL_MODES = {
    "shift": tnp.tone(tnp.SHIFT, 14), "window": tnp.tone(tnp.WINDOW, 14, lo=600, hi=9000),
    "percentile": tnp.tone(tnp.PERCENTILE, 14, p_lo=100, p_hi=100), "minmax": tnp.tone(tnp.PERCENTILE, 14),
    "equalize": tnp.tone(tnp.EQUALIZE, 14), "plateau": tnp.tone(tnp.EQUALIZE, 14, plateau=2),
    "table": tnp.tone(tnp.TABLE, 14, lut=np.random.default_rng(1).integers(0, 256, 65536).astype(np.uint8)),
}


@pytest.mark.parametrize("mode", list(GLOBAL_MODES))
def test_range_off_is_tone_np(mode):
    tm = GLOBAL_MODES[mode]
    px = tnp.over_depth(37, 23, seed=2)
    want = tnp.apply(px, tm)
    assert (vnp.apply(px, tm, vnp.OFF) == want).all()
    lut, pair = vnp.table(px, tm, vnp.OFF)
    ref, ref_pair = tnp.lut_of(tnp.pack16(px), 37, 23, tm)
    assert (lut == ref).all() and tuple(pair) == tuple(ref_pair)
    assert (vnp.mask(px, 1, vnp.OFF) == 1).all()


@pytest.mark.parametrize("tiles", [(1, 1), (3, 2), (8, 8)])
def test_range_off_is_clahe_np(tiles):
    px = cnp.halves(40, 24, seed=3)
    for plateau in (0, 2):
        tm = cnp.clahe(*tiles, plateau, 16)
        luts, n = vnp.tile_luts(px, tm, vnp.OFF)
        ref, ref_n = cnp.tile_luts(px, tm)
        assert (luts == ref).all() and (n == ref_n).all()
        assert (vnp.apply(px, tm, vnp.OFF) == cnp.apply(px, tm)).all()


@pytest.mark.parametrize("mode", list(GLOBAL_MODES))
def test_a_ranged_table_is_the_table_of_the_valid_pixels_alone(mode):
    """The valid pixels listed as a 1 x N frame give tone_np the same histogram: same table, same pair."""
    tm = GLOBAL_MODES[mode]
    px, rng, _ = vnp.depth_holes(37, 23, seed=4)
    kept = np.asarray(px)[vnp.valid(px, rng)][None, :]
    assert 0 < kept.size < px.size
    lut, pair = vnp.table(px, tm, rng)
    ref, ref_pair = tnp.table(tm, tnp.histogram(kept, tm["bits"]))
    assert (lut == ref).all() and tuple(pair) == tuple(ref_pair)
    assert (vnp.apply(px, tm, rng) == ref[px.astype(np.int64)]).all()      # invalid pixels go through the table too


@pytest.mark.parametrize("tiles", [(3, 2), (8, 8)])
def test_a_ranged_tile_table_is_clahe_np_of_the_tiles_valid_pixels(tiles):
    tx, ty = tiles
    px, rng, bits = vnp.depth_holes(40, 24, seed=5)
    for plateau in (0, 3):
        tm = cnp.clahe(tx, ty, plateau, bits)
        luts, n = vnp.tile_luts(px, tm, rng)
        tile = cnp.tile_map(40, 24, tx, ty)
        for t in range(tx * ty):
            kept = px[(tile == t) & vnp.valid(px, rng)][None, :]
            ref, ref_n = cnp.tables_of_histograms(tnp.histogram(kept, bits)[None, :], bits, plateau)
            assert (luts[t // tx, t % tx] == ref[0]).all() and n[t // tx, t % tx] == ref_n[0] == kept.size


def test_no_valid_pixel():
    px, rng, bits = vnp.nothing_valid(37, 23)
    for tm in (tnp.tone(tnp.PERCENTILE, bits, p_lo=50, p_hi=50), tnp.tone(tnp.PERCENTILE, bits), tnp.tone(tnp.EQUALIZE, bits),
               tnp.tone(tnp.EQUALIZE, bits, plateau=1)):
        lut, pair = vnp.table(px, tm, rng)
        assert (lut == 0).all() and tuple(pair) == (0, 0)
        assert (vnp.apply(px, tm, rng) == 0).all()
    for tm in (tnp.tone(tnp.SHIFT, bits), tnp.tone(tnp.WINDOW, bits, lo=5, hi=900)):                # no statistics: unchanged
        lut, pair = vnp.table(px, tm, rng)
        assert (lut == tnp.table(tm)[0]).all() and tuple(pair) == tuple(tnp.table(tm)[1])
    assert (vnp.mask(px, 1, rng) == 0).all()


def test_an_empty_tile_takes_the_shift_table():
    tx, ty = 3, 2
    for bits in (12, 16):
        px, rng, _ = vnp.empty_tile(40, 24, tx, ty, 1, 0, seed=6)
        tm = cnp.clahe(tx, ty, 2, bits)
        luts, n = vnp.tile_luts(px, tm, rng)
        assert n[0, 1] == 0 and (np.delete(n.ravel(), 1) > 0).all()
        m = (1 << bits) - 1
        assert (luts[0, 1] == (np.minimum(np.arange(65536), m) >> (bits - 8))).all()
        assert luts[0, 1][m] == 255 and luts[0, 1][0] == 0
        # its neighbours are cnp's of their own pixels, and a valid pixel beside the empty tile blends with a neutral table
        ref, _ = cnp.tile_luts(np.where(px == 0, 1200, px).astype(np.uint16), tm)
        assert (luts[1, 0] == ref[1, 0]).all()


@pytest.mark.parametrize("f", rnp.FACTORS)
def test_the_mask_rule(f):
    w, h = 9, 7
    px, rng, _ = vnp.block_corner(f * w, f * h, f, seed=f)
    ok = vnp.valid(px, rng)
    fm = (np.random.default_rng(f).random((h, w)) < 0.8).astype(np.uint8) * 7
    got, got_fm = vnp.mask(px, f, rng), vnp.mask(px, f, rng, fm)
    for y in range(h):
        for x in range(w):
            whole = bool(ok[f * y:f * y + f, f * x:f * x + f].all())
            assert got[y, x] == int(whole) and got_fm[y, x] == int(whole and fm[y, x] != 0)
    assert int((got == 0).sum()) == 4                                       # the four planted corners, a block each


def test_validity_is_tested_before_saturation():
    """(0, 4095) at bits 12 drops a 65535 that would otherwise count as 4095."""
    px, rng, bits = vnp.dead_pixels(40, 24, count=5, seed=7)
    assert vnp.histogram(px, bits, vnp.OFF)[4095] == 5 and vnp.histogram(px, bits, rng)[4095] == 0
    assert vnp.histogram(px, bits, rng).sum() == px.size - 5
    tm = tnp.tone(tnp.PERCENTILE, bits)
    assert vnp.table(px, tm, vnp.OFF)[1][1] == 4095 and vnp.table(px, tm, rng)[1][1] <= 3000
    assert (vnp.apply(px, tm, rng)[px == 65535] == 255).all()               # still table[min(raw, M)]


@pytest.mark.parametrize("content", ["depth_holes", "dead_pixels", "lone_sentinel"])
def test_a_float64_model_of_the_quotients_agrees(content):
    px, rng, bits = getattr(vnp, content)(37, 23, seed=8)
    tm = tnp.tone(tnp.EQUALIZE, bits)
    assert (vnp.float_tables(px, tm, rng) == vnp.table(px, tm, rng)[0]).all()
    tm = cnp.clahe(3, 2, 0, bits)
    assert (vnp.float_tables(px, tm, rng) == vnp.tile_luts(px, tm, rng)[0]).all()
    px, rng, bits = vnp.empty_tile(40, 24, 3, 2, 2, 1, seed=9)
    tm = cnp.clahe(3, 2, 0, bits)
    assert (vnp.float_tables(px, tm, rng) == vnp.tile_luts(px, tm, rng)[0]).all()


@pytest.mark.parametrize("name", list(cases.FRAMES))
def test_premises_of_the_planted_frames(name):
    """Every frame the GPU tests plant, at every size and factor they use it: the ranged table differs from the unranged one under
    each data-dependent mode, and the mask has both values (the frame with no valid pixel: all 0, which all-1 cannot match)."""
    for (w, h) in cases.SIZES:
        for f in cases.FRAMES[name]["factors"]:
            px, rng, bits = cases.frame(name, w, h, f)
            assert px.shape == (f * h, f * w) and px.dtype == np.uint16 and vnp.is_on(rng)
            m = vnp.mask(px, f, rng)
            assert (m == 0).any()
            assert (m == 1).any() or name == "nothing_valid"
            for tm in cases.tone_maps(bits, w * f, h * f):
                if not vnp.from_frame(tm) or tm["label"] in cases.FRAMES[name]["same_under"]:
                    continue
                if vnp.tiled(tm):
                    differ = (vnp.tile_luts(px, tm, rng)[0] != vnp.tile_luts(px, tm, vnp.OFF)[0]).any()
                else:
                    differ = (vnp.table(px, tm, rng)[0] != vnp.table(px, tm, vnp.OFF)[0]).any()
                assert differ, (name, w, h, f, tm)
