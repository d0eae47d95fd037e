"""CPU checks of the deep raw formats' models (tests/helpers/packed_np.py) and of nmi_frame_row_bytes: the bit-string model and the
byte formulas agree, the known answers of the standards' layouts come out, pack then unpack is the identity, the 16-bit mosaic
rule ties to the 8-bit one and does not overflow, and the library's row bytes are the models'.  No device is needed."""
import ctypes as C

import numpy as np
import pytest

from helpers import packed_np as pnp
from helpers import sensor_np as snp
from orbslam2_nmi_amd import capi

# (pixels, format, bytes): include/nmi_hip.h "Deep frames", from the PFNC and CSI-2 / V4L2 layouts
KNOWN = [((0x3FF, 0x000, 0x155, 0x2AA), pnp.MONO10P, "FF 03 50 95 AA"),
         ((0x3FF, 0x000, 0x155, 0x2AA), pnp.RAW10, "FF 00 55 AA 93"),
         ((0x001, 0x200, 0x0F3, 0x30C), pnp.MONO10P, "01 00 38 0F C3"),
         ((0x001, 0x200, 0x0F3, 0x30C), pnp.RAW10, "00 80 3C C3 31"),
         ((0xABC, 0x123), pnp.MONO12P, "BC 3A 12"),
         ((0xABC, 0x123), pnp.RAW12, "AB 12 3C"),
         ((0x1234, 0x00FF), pnp.GRAY16_BE, "12 34 00 FF")]


def test_ids_and_constants():
    assert (capi.FRAME_GRAY16_BE, capi.FRAME_MONO10P, capi.FRAME_MONO12P, capi.FRAME_RAW10, capi.FRAME_RAW12) == pnp.LAYOUTS
    assert (capi.FRAME_BAYER16_RGGB, capi.FRAME_BAYER16_GRBG, capi.FRAME_BAYER16_GBRG, capi.FRAME_BAYER16_BGGR) == pnp.BAYER16_IDS
    assert capi.FRAME_UNPACKED == pnp.FORMATS and capi.FRAME_GRAY16 == pnp.GRAY16
    # the ids other tests hold unknown stay clear of the new ones
    unknown = {-1, 36, 47, 49, 99} | set(range(5, 16)) | set(range(18, 32))
    assert not unknown & set(pnp.FORMATS)


@pytest.mark.parametrize("px,fmt,text", KNOWN)
def test_known_answers(px, fmt, text):
    want = np.array([int(t, 16) for t in text.split()], np.uint8)
    row = np.array([px], np.uint16)
    assert (pnp.pack_row_bits(px, fmt) == want).all()
    assert (pnp.pack_rows(row, fmt)[0] == want).all()
    assert (pnp.unpack_row_bits(want, fmt, len(px)) == row[0]).all()
    assert (pnp.unpack_rows(want[None], fmt, len(px)) == row).all()


@pytest.mark.parametrize("fmt", pnp.LAYOUTS)
@pytest.mark.parametrize("w", [4, 8, 12, 20, 52])
def test_the_two_models_agree_and_round_trip(fmt, w):
    px = pnp.random_pixels(fmt, w, 6, seed=w + fmt)
    px[0], px[1] = 0, (1 << pnp.BITS[fmt]) - 1
    rows = pnp.pack_rows(px, fmt)
    assert rows.shape == (6, pnp.row_bytes(fmt, w))
    for y in range(6):
        assert (pnp.pack_row_bits(px[y], fmt) == rows[y]).all()
        assert (pnp.unpack_row_bits(rows[y], fmt, w) == px[y]).all()
    assert (pnp.unpack_rows(rows, fmt, w) == px).all()
    # every byte pattern is some row: unpack then pack is the identity too
    junk = np.random.default_rng(w).integers(0, 256, rows.shape, dtype=np.uint8)
    assert (pnp.pack_rows(pnp.unpack_rows(junk, fmt, w), fmt) == junk).all()


@pytest.mark.parametrize("fmt", pnp.FORMATS)
def test_frames_read_back_and_ignore_the_junk(fmt):
    w, h = 12, 5
    px = pnp.random_pixels(fmt, w, h, seed=3)
    dense = pnp.container(pnp.frame(px, fmt), fmt, w, h)
    step = 2 if pnp.GROUP[fmt][1] == 2 else 3
    for seed in (1, 2):
        buf = pnp.frame(px, fmt, pnp.row_bytes(fmt, w) + step, 2, seed)
        assert buf.size == 2 + pnp.span(fmt, w, h, pnp.row_bytes(fmt, w) + step)
        assert (pnp.container(buf, fmt, w, h, pnp.row_bytes(fmt, w) + step, 2) == dense).all()
    if fmt not in pnp.BAYER16_IDS:
        assert (dense == px).all()


@pytest.mark.parametrize("name", list(pnp.BAYER16))
def test_bayer16_ties_to_the_8_bit_rule(name):
    fmt = pnp.BAYER16[name]
    for w, h in ((2, 2), (3, 2), (13, 7)):
        m = np.random.default_rng(w * h).integers(0, 256, (h, w))
        assert (pnp.bayer16_gray(m, fmt) == snp.bayer_gray(m, snp.BAYER_FORMATS[name])).all()
        assert (pnp.bayer16_gray(np.full((h, w), 65535), fmt) == 65535).all()       # saturated, no overflow
        assert (pnp.bayer16_gray(np.full((h, w), 4321), fmt) == 4321).all()         # a flat mosaic of g gives g
    assert 16384 * 4 * 65535 + 32768 < 2 ** 32


def test_row_bytes_of_the_library():
    lib = capi.load_library()
    assert lib.nmi_frame_row_bytes.restype is C.c_int64
    for fmt in pnp.FORMATS:
        for w in (0, 2, 4, 6, 8, 50):
            want = pnp.row_bytes(fmt, w)
            assert lib.nmi_frame_row_bytes(fmt, w) == want == capi.frame_row_bytes(fmt, w), (fmt, w)
    assert [capi.frame_row_bytes(pnp.MONO10P, w) for w in (0, 2, 4, 6, 8, 50)] == [0, 0, 5, 0, 10, 0]
    assert [capi.frame_row_bytes(pnp.RAW12, w) for w in (0, 2, 4, 6, 8, 50)] == [0, 3, 6, 9, 12, 75]
    assert [capi.frame_row_bytes(pnp.GRAY16_BE, w) for w in (0, 2, 4, 6, 8, 50)] == [0, 4, 8, 12, 16, 100]
    # the formats there already were: width * bytes per pixel; unknown ids: 0
    for fmt, bpp in capi.FRAME_BYTES_PER_PIXEL.items():
        assert capi.frame_row_bytes(fmt, 50) == 50 * bpp and capi.frame_row_bytes(fmt, -3) == 0
    for fmt in (-1, 5, 15, 18, 31, 36, 47, 49, 51, 60, 99):
        assert capi.frame_row_bytes(fmt, 8) == 0
