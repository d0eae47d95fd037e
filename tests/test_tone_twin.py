"""CPU checks of the numpy twin of the deep grey frames (tests/helpers/tone_np.py; rule: include/nmi_hip.h "Deep frames"): the
properties the rule promises, and a float64 model of every quotient."""
import numpy as np
import pytest

from helpers import tone_np as tnp

W, H = 40, 24
CONTENTS = {"uniform": lambda: tnp.uniform(W, H, 1), "flat": lambda: tnp.flat(W, H), "two": lambda: tnp.two_valued(W, H),
            "thermal": lambda: tnp.thermal(W, H, 2), "over": lambda: tnp.over_depth(W, H, 3)}
TONES = {"shift16": tnp.tone(tnp.SHIFT, 16), "shift12": tnp.tone(tnp.SHIFT, 12), "window": tnp.tone(tnp.WINDOW, 14, lo=7000, hi=7400),
         "minmax": tnp.tone(tnp.PERCENTILE, 16), "pct": tnp.tone(tnp.PERCENTILE, 14, p_lo=100, p_hi=250),
         "eq": tnp.tone(tnp.EQUALIZE, 16), "eq12": tnp.tone(tnp.EQUALIZE, 12), "plateau": tnp.tone(tnp.EQUALIZE, 14, plateau=3)}


def table_of(px, tm):
    return tnp.table(tm, tnp.histogram(px, tm["bits"]))


@pytest.mark.parametrize("content", list(CONTENTS))
@pytest.mark.parametrize("name", list(TONES))
def test_every_table_is_non_decreasing(content, name):
    lut, (lo, hi) = table_of(CONTENTS[content](), TONES[name])
    assert lut.shape == (tnp.LEVELS,) and lut.dtype == np.uint8
    assert (np.diff(lut.astype(np.int64)) >= 0).all()
    m = (1 << TONES[name]["bits"]) - 1
    assert 0 <= lo <= hi <= m and (lut[m:] == lut[m]).all()


@pytest.mark.parametrize("bits", [8, 10, 12, 14, 16])
def test_shift_is_the_shift(bits):
    lut, pair = tnp.table(tnp.tone(tnp.SHIFT, bits))
    m = (1 << bits) - 1
    v = np.minimum(np.arange(tnp.LEVELS), m)
    assert (lut == v >> (bits - 8)).all() and pair == (0, m) and lut[m] == 255


def test_window_ends_and_midpoint():
    lut, pair = tnp.table(tnp.tone(tnp.WINDOW, 16, lo=1000, hi=3000))
    assert pair == (1000, 3000)
    assert lut[1000] == 0 and lut[1001] == 0 and lut[999] == 0 and lut[0] == 0
    assert lut[3000] == 255 and lut[65535] == 255
    assert lut[2000] == 128          # (1000 * 255 + 1000) // 2000 = 128: the half rounds up
    assert lut[2999] == 255 and lut[1004] == 1


def test_equalize_of_every_value_once():
    px = np.arange(65536, dtype=np.uint16).reshape(256, 256)
    lut, pair = table_of(px, tnp.tone(tnp.EQUALIZE, 16))
    v = np.arange(65536, dtype=np.int64)
    assert (lut == (v * 255 + 32767) // 65535).all() and pair == (0, 65535)


@pytest.mark.parametrize("content", ["uniform", "two", "thermal"])
def test_percentile_zero_is_min_max(content):
    px = CONTENTS[content]()
    lut, pair = table_of(px, tnp.tone(tnp.PERCENTILE, 16))
    assert pair == (int(px.min()), int(px.max()))
    want, _ = tnp.table(tnp.tone(tnp.WINDOW, 16, lo=pair[0], hi=pair[1]))
    assert (lut == want).all()


def test_a_flat_frame_is_all_zero():
    px = tnp.flat(W, H, 7123)
    for tm in (tnp.tone(tnp.PERCENTILE, 16), tnp.tone(tnp.PERCENTILE, 14, p_lo=300, p_hi=300), tnp.tone(tnp.EQUALIZE, 16),
               tnp.tone(tnp.EQUALIZE, 14, plateau=5)):
        assert (tnp.apply(px, tm) == 0).all()
        assert table_of(px, tm)[1] == (7123, 7123)


def test_plateau_one_depends_on_presence_only():
    rng = np.random.default_rng(5)
    values = rng.choice(16384, size=50, replace=False)
    a = rng.choice(values, size=W * H)
    a[:50] = values
    b = np.concatenate([values, np.full(W * H - 50, values[0])])
    tm = tnp.tone(tnp.EQUALIZE, 14, plateau=1)
    la, lb = table_of(a, tm)[0], table_of(b, tm)[0]
    assert (la == lb).all()
    assert (la != table_of(a, tnp.tone(tnp.EQUALIZE, 14))[0]).any()      # (the counts matter without the plateau)
    assert (la[np.sort(values)] == (np.arange(50) * 255 + 24) // 49).all()   # h' = 1 each: c0 = 1, T = 50


def test_saturation_at_12_bits():
    px = tnp.over_depth(W, H, 3)
    assert px.max() > 4095
    clipped = np.minimum(px, 4095)
    for name in ("shift12", "eq12"):
        tm = TONES[name]
        assert (tnp.apply(px, tm) == tnp.apply(clipped, tm)).all()
    assert (tnp.apply(px, TONES["shift12"])[px >= 4095] == 255).all()
    h = tnp.histogram(px, 12)
    assert h[4096:].sum() == 0 and h.sum() == px.size and h[4095] == (px >= 4095).sum()


def round_half_up(q):
    return np.floor(q + 0.5)


@pytest.mark.parametrize("content", list(CONTENTS))
@pytest.mark.parametrize("name", ["window", "minmax", "pct", "eq", "eq12", "plateau"])
def test_the_twin_agrees_with_a_float_model(content, name):
    px, tm = CONTENTS[content](), TONES[name]
    bits = tm["bits"]
    m = (1 << bits) - 1
    h = tnp.histogram(px, bits)
    lut, (lo, hi) = tnp.table(tm, h)
    v = np.minimum(np.arange(tnp.LEVELS), m).astype(np.float64)
    if tm["mode"] == tnp.EQUALIZE:
        hc = np.minimum(h, tm["plateau"]) if tm["plateau"] else h
        c = np.cumsum(hc).astype(np.float64)
        t, c0 = c[m], float(hc[lo])
        if t == c0:
            assert (lut == 0).all()
            return
        q = np.where(v >= lo, (c[v.astype(np.int64)] - c0) * 255.0 / (t - c0), 0.0)
    else:
        if hi == lo:                      # a flat frame: its one value (and all below) 0, by the order of the cases
            assert (lut[:lo + 1] == 0).all() and (lut[lo + 1:] == 255).all()
            return
        q = np.clip((v - lo) * 255.0 / (hi - lo), 0.0, 255.0)
    sure = np.abs(q - np.floor(q) - 0.5) > 1e-9
    assert sure.sum() > tnp.LEVELS // 2
    assert (lut[sure] == round_half_up(q[sure])).all()


def test_pack16_round_trips_and_pads_with_noise():
    px = tnp.uniform(5, 3, 9)
    for pitch, off in ((0, 0), (12, 2), (74, 6)):
        buf = tnp.pack16(px, pitch, off, seed=1)
        assert buf.size == off + tnp.span(5, 3, pitch)
        assert (tnp.pixels(buf, 5, 3, pitch, off) == px).all()
        assert (tnp.to_gray(buf, 5, 3, tnp.tone(), pitch, off) == px >> 8).all()
    big = tnp.uniform(10, 6, 4)
    buf = tnp.pack16(big, 26, 2)
    got = tnp.reduce_frame(buf, 5, 3, 2, tnp.tone(), 26, 2)
    s = (big >> 8).astype(np.int64).reshape(3, 2, 5, 2).sum(axis=(1, 3))
    assert (got == (s + 2) >> 2).all()
