"""numpy restatement of the raw sensor formats of nmi_gray_frame (include/nmi_hip.h) -- TEST INFRASTRUCTURE ONLY.

Packed YUV 4:2:2 (YUYV, UYVY): the grey value is the luma byte.  Bayer mosaics (RGGB, GRBG, GBRG, BGGR: the 2x2 tile at (0, 0)):
a bilinear demosaic with reflected edges (-1 -> 1, W -> W - 2) and the grey weights with one rounding, in int64:
    gray = (4899 R4 + 9617 G4 + 1868 B4 + 32768) >> 16
pack() lays a frame out in a format (and a pitch, behind an offset) with junk in every byte the rule must not read; mosaic()
samples an RGB image into a mosaic; to_gray() is the rule on such a buffer and reduce_frame() chains it into
helpers/reduce_np.py, undistorted() into helpers/undistort_np.py.
"""
import numpy as np

from helpers import reduce_np as rnp

YUYV, UYVY = 16, 17
RGGB, GRBG, GBRG, BGGR = 32, 33, 34, 35
YUV_FORMATS = {"yuyv": YUYV, "uyvy": UYVY}
BAYER_FORMATS = {"rggb": RGGB, "grbg": GRBG, "gbrg": GBRG, "bggr": BGGR}
FORMATS = {**YUV_FORMATS, **BAYER_FORMATS}
BPP = {YUYV: 2, UYVY: 2, RGGB: 1, GRBG: 1, GBRG: 1, BGGR: 1}
LUMA_BYTE = {YUYV: 0, UYVY: 1}
RED_SITE = {RGGB: (0, 0), GRBG: (1, 0), GBRG: (0, 1), BGGR: (1, 1)}   # (x & 1, y & 1) of the red sites


def is_bayer(fmt):
    return fmt in RED_SITE


def row_bytes(fmt, w, pitch=0):
    return pitch if pitch else w * BPP[fmt]


def span(fmt, w, h, pitch=0):
    """Bytes from the first pixel to the end of the last row's pixels: (H - 1) * pitch + W * bpp."""
    return (h - 1) * row_bytes(fmt, w, pitch) + w * BPP[fmt]


def mosaic(rgb, fmt):
    """[H,W,3] RGB uint8 -> [H,W] mosaic: each site keeps the channel its pattern gives it."""
    h, w = rgb.shape[:2]
    rx, ry = RED_SITE[fmt]
    yy, xx = np.mgrid[0:h, 0:w]
    a, b = (xx & 1) ^ rx, (yy & 1) ^ ry
    chan = np.where(a != b, 1, np.where(a == 0, 0, 2))
    return np.take_along_axis(np.asarray(rgb, np.uint8), chan[..., None], axis=2)[..., 0]


def demosaic4(m, fmt):
    """[H,W] mosaic -> (R4, G4, B4), int64: four times the bilinear channels, edges reflected without repeating them."""
    m = np.asarray(m, np.int64)
    h, w = m.shape
    assert h >= 2 and w >= 2
    p = np.pad(m, 1, mode="reflect")

    def at(dx, dy):
        return p[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]

    c = at(0, 0)
    hs, vs = at(-1, 0) + at(1, 0), at(0, -1) + at(0, 1)
    ds = at(-1, -1) + at(1, -1) + at(-1, 1) + at(1, 1)
    rx, ry = RED_SITE[fmt]
    yy, xx = np.mgrid[0:h, 0:w]
    a, b = (xx & 1) ^ rx, (yy & 1) ^ ry
    red, blue, g_red_row = (a == 0) & (b == 0), (a == 1) & (b == 1), (a == 1) & (b == 0)
    r4 = np.where(red, 4 * c, np.where(blue, ds, np.where(g_red_row, 2 * hs, 2 * vs)))
    b4 = np.where(blue, 4 * c, np.where(red, ds, np.where(g_red_row, 2 * vs, 2 * hs)))
    g4 = np.where(red | blue, hs + vs, 4 * c)
    return r4, g4, b4


def bayer_gray(m, fmt):
    """The Bayer rule on a mosaic [H,W] -> [H,W] uint8."""
    r4, g4, b4 = demosaic4(m, fmt)
    return ((4899 * r4 + 9617 * g4 + 1868 * b4 + 32768) >> 16).astype(np.uint8)


def pack(img, fmt, pitch=0, offset=0, seed=0):
    """img: [H,W] uint8, the luma plane (YUV) or the mosaic (Bayer) -> flat uint8 buffer: `offset` junk bytes, then the H rows of
    `pitch` bytes in fmt.  The offset, the pitch's padding and the chroma bytes hold random junk: the rule must not read them."""
    h, w = img.shape
    bpp, rb = BPP[fmt], row_bytes(fmt, w, pitch)
    rng = np.random.default_rng(seed)
    buf = rng.integers(0, 256, offset + (h - 1) * rb + w * bpp, dtype=np.uint8)
    for y in range(h):
        o = offset + y * rb
        if bpp == 2:
            buf[o + LUMA_BYTE[fmt]:o + 2 * w:2] = img[y]
        else:
            buf[o:o + w] = img[y]
    return buf


def pixels(buf, fmt, w, h, pitch=0, offset=0):
    """The luma plane or mosaic [H,W] of a flat buffer laid out as pack() lays it out."""
    rb, bpp = row_bytes(fmt, w, pitch), BPP[fmt]
    buf = np.asarray(buf, np.uint8)
    first = LUMA_BYTE.get(fmt, 0)
    return np.stack([buf[offset + y * rb + first: offset + y * rb + w * bpp: bpp] for y in range(h)])


def to_gray(buf, fmt, w, h, pitch=0, offset=0):
    """The rule on a flat buffer laid out as pack() lays it out -> [H,W] uint8.  Only the w x h pixels are read: a wider pitch
    crops, and the last column and row reflect inwards."""
    px = pixels(buf, fmt, w, h, pitch, offset)
    return bayer_gray(px, fmt) if is_bayer(fmt) else px.copy()


def reduce_frame(buf, fmt, w, h, f, pitch=0, offset=0):
    """nmi_reduce_frame on a buffer of f*h rows of f*w pixels -> [h, w] uint8: the grey rule, then reduce_np's box rule."""
    return rnp.reduce_gray(to_gray(buf, fmt, f * w, f * h, pitch, offset), f)


def chroma_frame(w, h, seed=0):
    """[H,W,3] RGB uint8 with strong, smoothly varying chroma, so that pattern and channel order matter."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    ph = rng.uniform(0, 2 * np.pi, 3)
    r = 128 + 100 * np.sin(xx / 7.0 + ph[0])
    g = 128 + 100 * np.sin(yy / 5.0 + ph[1])
    b = 128 + 100 * np.sin((xx + yy) / 9.0 + ph[2])
    return np.clip(np.stack([r, g, b], -1) + rng.integers(-20, 21, (h, w, 3)), 0, 255).astype(np.uint8)
