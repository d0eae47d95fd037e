"""numpy / Python-integer restatement of the deep raw formats (include/nmi_hip.h "Deep frames") -- TEST INFRASTRUCTURE ONLY.

Each format unpacks to a 16-bit container pixel u(x, y).  The five byte layouts are written twice, by two different readings of
the standards: as a bit string (a row is one little-endian Python integer, pixel k a bit field of it: PFNC's "lsb packed"; the
CSI-2 layouts as their own fields) and from the byte formulas of the header's table (numpy).  tests/test_packed_twin.py holds
the two against each other and against known answers.  The 16-bit mosaics' grey value is sensor_np's demosaic, in int64, without
its cast to 8 bits.  frame() lays a container out in a format behind an offset and with a pitch, with junk in every byte the
rule must not read; container() reads such a buffer back."""
import numpy as np

from helpers import sensor_np as snp

GRAY16 = 48
GRAY16_BE, MONO10P, MONO12P, RAW10, RAW12 = 50, 52, 53, 54, 55
BAYER16 = {"rggb": 56, "grbg": 57, "gbrg": 58, "bggr": 59}
BAYER16_IDS = tuple(BAYER16.values())
LAYOUTS = (GRAY16_BE, MONO10P, MONO12P, RAW10, RAW12)
PACKED = (MONO10P, MONO12P, RAW10, RAW12)
FORMATS = LAYOUTS + BAYER16_IDS
BITS = {GRAY16_BE: 16, MONO10P: 10, MONO12P: 12, RAW10: 10, RAW12: 12, **{f: 16 for f in BAYER16_IDS}}
GROUP = {GRAY16_BE: (1, 2), MONO10P: (4, 5), MONO12P: (2, 3), RAW10: (4, 5), RAW12: (2, 3), **{f: (1, 2) for f in BAYER16_IDS}}  # pixels, bytes
# the 8-bit mosaic with the same pattern (sensor_np's ids)
BAYER8 = {BAYER16[k]: snp.BAYER_FORMATS[k] for k in BAYER16}


def row_bytes(fmt, w):
    """Dense bytes of a row of w pixels; 0 for an unknown format, w <= 0 or a width that is not whole groups."""
    if fmt not in GROUP or w <= 0:
        return 0
    px, by = GROUP[fmt]
    return w // px * by if w % px == 0 else 0


def span(fmt, w, h, pitch=0):
    return (h - 1) * (pitch or row_bytes(fmt, w)) + row_bytes(fmt, w)


# --- the bit-string model (Python integers) -----------------------------------------------------------------------------------------

def pack_row_bits(px, fmt):
    """One row of pixels -> bytes, through one little-endian integer."""
    px = [int(v) for v in px]
    n = row_bytes(fmt, len(px))
    assert n > 0 and all(0 <= v < (1 << BITS[fmt]) for v in px)
    s = 0
    if fmt in (MONO10P, MONO12P):                      # pixel k is bits [bits k, bits k + bits)
        for k, v in enumerate(px):
            s |= v << (BITS[fmt] * k)
    elif fmt == GRAY16_BE:                             # the high byte first
        for k, v in enumerate(px):
            s |= ((v >> 8) | ((v & 255) << 8)) << (16 * k)
    elif fmt == RAW10:                                 # per 40-bit group: four high bytes, then four 2-bit fields, pixel 0's lowest
        for k, v in enumerate(px):
            g, i = divmod(k, 4)
            s |= (v >> 2) << (40 * g + 8 * i)
            s |= (v & 3) << (40 * g + 32 + 2 * i)
    else:                                              # RAW12, per 24-bit group: two high bytes, then two 4-bit fields
        for k, v in enumerate(px):
            g, i = divmod(k, 2)
            s |= (v >> 4) << (24 * g + 8 * i)
            s |= (v & 15) << (24 * g + 16 + 4 * i)
    return np.frombuffer(s.to_bytes(n, "little"), np.uint8).copy()


def unpack_row_bits(b, fmt, w):
    s = int.from_bytes(bytes(np.asarray(b, np.uint8)[:row_bytes(fmt, w)]), "little")
    out = []
    for k in range(w):
        if fmt in (MONO10P, MONO12P):
            out.append((s >> (BITS[fmt] * k)) & ((1 << BITS[fmt]) - 1))
        elif fmt == GRAY16_BE:
            v = (s >> (16 * k)) & 0xFFFF
            out.append((v >> 8) | ((v & 255) << 8))
        elif fmt == RAW10:
            g, i = divmod(k, 4)
            out.append((((s >> (40 * g + 8 * i)) & 255) << 2) | ((s >> (40 * g + 32 + 2 * i)) & 3))
        else:
            g, i = divmod(k, 2)
            out.append((((s >> (24 * g + 8 * i)) & 255) << 4) | ((s >> (24 * g + 16 + 4 * i)) & 15))
    return np.array(out, np.uint16)


# --- the byte formulas of the header's table (numpy, whole frames) ---------------------------------------------------------------------

def pack_rows(px, fmt):
    """[H,W] pixels -> [H, row bytes] uint8."""
    p = np.asarray(px, np.int64)
    h, w = p.shape
    assert row_bytes(fmt, w) > 0 and p.min() >= 0 and p.max() < (1 << BITS[fmt])
    b = np.zeros((h, row_bytes(fmt, w)), np.int64)
    if fmt == GRAY16_BE:
        b[:, 0::2], b[:, 1::2] = p >> 8, p & 255
    elif fmt == MONO10P:     # p0 | p1 << 10 | p2 << 20 | p3 << 30, cut into five bytes
        p0, p1, p2, p3 = (p[:, i::4] for i in range(4))
        b[:, 0::5] = p0 & 255
        b[:, 1::5] = (p0 >> 8) | ((p1 & 63) << 2)
        b[:, 2::5] = (p1 >> 6) | ((p2 & 15) << 4)
        b[:, 3::5] = (p2 >> 4) | ((p3 & 3) << 6)
        b[:, 4::5] = p3 >> 2
    elif fmt == MONO12P:
        p0, p1 = p[:, 0::2], p[:, 1::2]
        b[:, 0::3] = p0 & 255
        b[:, 1::3] = (p0 >> 8) | ((p1 & 15) << 4)
        b[:, 2::3] = p1 >> 4
    elif fmt == RAW10:
        for i in range(4):
            b[:, i::5] = p[:, i::4] >> 2
            b[:, 4::5] |= (p[:, i::4] & 3) << (2 * i)
    else:
        b[:, 0::3], b[:, 1::3] = p[:, 0::2] >> 4, p[:, 1::2] >> 4
        b[:, 2::3] = (p[:, 0::2] & 15) | ((p[:, 1::2] & 15) << 4)
    return b.astype(np.uint8)


def unpack_rows(rows, fmt, w):
    """[H, >= row bytes] uint8 -> [H,W] uint16 by the table's formulas."""
    b = np.asarray(rows, np.uint8)[:, :row_bytes(fmt, w)].astype(np.int64)
    u = np.zeros((b.shape[0], w), np.int64)
    if fmt == GRAY16_BE:
        u = (b[:, 0::2] << 8) | b[:, 1::2]
    elif fmt == MONO10P:
        b0, b1, b2, b3, b4 = (b[:, i::5] for i in range(5))
        u[:, 0::4] = b0 | ((b1 & 3) << 8)
        u[:, 1::4] = (b1 >> 2) | ((b2 & 15) << 6)
        u[:, 2::4] = (b2 >> 4) | ((b3 & 63) << 4)
        u[:, 3::4] = (b3 >> 6) | (b4 << 2)
    elif fmt == MONO12P:
        b0, b1, b2 = (b[:, i::3] for i in range(3))
        u[:, 0::2] = b0 | ((b1 & 15) << 8)
        u[:, 1::2] = (b1 >> 4) | (b2 << 4)
    elif fmt == RAW10:
        for i in range(4):
            u[:, i::4] = (b[:, i::5] << 2) | ((b[:, 4::5] >> (2 * i)) & 3)
    else:
        u[:, 0::2] = (b[:, 0::3] << 4) | (b[:, 2::3] & 15)
        u[:, 1::2] = (b[:, 1::3] << 4) | (b[:, 2::3] >> 4)
    return u.astype(np.uint16)


# --- 16-bit mosaics ------------------------------------------------------------------------------------------------------------------

def bayer16_gray(m, fmt):
    """The mosaic rule on raw 16-bit sites [H,W] -> the container [H,W] uint16: sensor_np's bilinear sums, int64, one rounding."""
    r4, g4, b4 = snp.demosaic4(np.asarray(m, np.int64), BAYER8[fmt])
    v = 4899 * r4 + 9617 * g4 + 1868 * b4 + 32768
    assert v.max() < 2 ** 32
    return (v >> 16).astype(np.uint16)


# --- frames --------------------------------------------------------------------------------------------------------------------------

def frame(px, fmt, pitch=0, offset=0, seed=0):
    """[H,W] pixels (a mosaic: its raw sites) -> flat uint8 buffer: `offset` junk bytes, then H rows of `pitch` bytes in fmt; the
    offset and the pitch's padding hold junk.  Nothing follows the last row's last byte."""
    px = np.asarray(px)
    h, w = px.shape
    rows = np.ascontiguousarray(px, "<u2").view(np.uint8).reshape(h, 2 * w) if fmt in BAYER16_IDS else pack_rows(px, fmt)
    n = rows.shape[1]
    rb = pitch or n
    assert rb >= n
    buf = np.random.default_rng(seed).integers(0, 256, offset + (h - 1) * rb + n, dtype=np.uint8)
    for y in range(h):
        buf[offset + y * rb:offset + y * rb + n] = rows[y]
    return buf


def container(buf, fmt, w, h, pitch=0, offset=0):
    """The dense container [H,W] uint16 of a buffer laid out as frame() lays it out: the model of nmi_unpack_frame."""
    n = row_bytes(fmt, w)
    rb = pitch or n
    buf = np.asarray(buf, np.uint8)
    rows = np.stack([buf[offset + y * rb:offset + y * rb + n] for y in range(h)])
    if fmt in BAYER16_IDS:
        sites = rows[:, 0::2].astype(np.uint16) | (rows[:, 1::2].astype(np.uint16) << 8)
        return bayer16_gray(sites, fmt)
    return unpack_rows(rows, fmt, w)


def random_pixels(fmt, w, h, seed=0):
    return np.random.default_rng(seed).integers(0, 1 << BITS[fmt], (h, w)).astype(np.uint16)


def contents(fmt, w, h, seed=0):
    """name -> [H,W] pixels: random, all ones, all zero, and random rows that each end in the maximum value (a read past the row,
    or a dropped tail run, changes the result)."""
    top = (1 << BITS[fmt]) - 1
    tail = random_pixels(fmt, w, h, seed + 1) >> 1
    tail[:, -1] = top
    return {"random": random_pixels(fmt, w, h, seed), "ones": np.full((h, w), top, np.uint16), "zeros": np.zeros((h, w), np.uint16),
            "tail": tail}
