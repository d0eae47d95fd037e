"""numpy restatement of the colour-to-grey rule (nmi_gray_frame, include/nmi_hip.h) -- TEST INFRASTRUCTURE ONLY.

gray = (4899 R + 9617 G + 1868 B + 8192) >> 14 per pixel of a frame held as H rows of `pitch` bytes (0: dense) in one of the
NMI_FRAME_* formats; GRAY with a pitch copies the rows.  pack() lays a frame out in a format (and a pitch, behind an offset)
the way a camera driver or a cv::Mat ROI would; colorize() makes a colour frame whose channels differ smoothly around a grey
image, so that the channel order matters; undistorted() chains the rule into helpers/undistort_np.py.
"""
import numpy as np

from helpers import undistort_np as unp

GRAY, BGR, RGB, BGRA, RGBA = 0, 1, 2, 3, 4
FORMATS = {"gray": GRAY, "bgr": BGR, "rgb": RGB, "bgra": BGRA, "rgba": RGBA}
COLOR_FORMATS = (BGR, RGB, BGRA, RGBA)
BPP = {GRAY: 1, BGR: 3, RGB: 3, BGRA: 4, RGBA: 4}
R_BYTE = {BGR: 2, RGB: 0, BGRA: 2, RGBA: 0}   # B is byte 2 - R_BYTE, G byte 1, alpha (4 channels) byte 3


def gray_of(r, g, b):
    """The rule on arrays of channel values -> uint8."""
    r, g, b = (np.asarray(c, np.int64) for c in (r, g, b))
    return ((4899 * r + 9617 * g + 1868 * b + 8192) >> 14).astype(np.uint8)


def row_bytes(fmt, w, pitch=0):
    return pitch if pitch else w * BPP[fmt]


def span(fmt, w, h, pitch=0):
    """Bytes from the first pixel to the end of the last row's pixels: (H - 1) * pitch + W * bpp."""
    return (h - 1) * row_bytes(fmt, w, pitch) + w * BPP[fmt]


def pack(img, fmt, pitch=0, offset=0, seed=0):
    """img: [H,W] grey (fmt GRAY) or [H,W,3] RGB uint8 -> flat uint8 buffer: `offset` junk bytes, then the H rows of `pitch` bytes in
    fmt.  Bytes outside the pixels (the offset, the pitch's padding, alpha) hold random junk: the rule must not read them."""
    h, w = img.shape[:2]
    rb = row_bytes(fmt, w, pitch)
    rng = np.random.default_rng(seed)
    buf = rng.integers(0, 256, offset + (h - 1) * rb + w * BPP[fmt], dtype=np.uint8)
    if fmt == GRAY:
        px = img.reshape(h, w, 1)
    else:
        px = np.empty((h, w, BPP[fmt]), np.uint8)
        ri = R_BYTE[fmt]
        px[..., ri], px[..., 1], px[..., 2 - ri] = img[..., 0], img[..., 1], img[..., 2]
        if BPP[fmt] == 4:
            px[..., 3] = rng.integers(0, 256, (h, w), dtype=np.uint8)
    for y in range(h):
        o = offset + y * rb
        buf[o:o + w * BPP[fmt]] = px[y].reshape(-1)
    return buf


def to_gray(buf, fmt, w, h, pitch=0, offset=0):
    """The rule on a flat buffer laid out as pack() lays it out -> [H,W] uint8."""
    rb, bpp = row_bytes(fmt, w, pitch), BPP[fmt]
    buf = np.asarray(buf, np.uint8)
    rows = np.stack([buf[offset + y * rb: offset + y * rb + w * bpp] for y in range(h)]).reshape(h, w, bpp)
    if fmt == GRAY:
        return rows[..., 0].copy()
    ri = R_BYTE[fmt]
    return gray_of(rows[..., ri], rows[..., 1], rows[..., 2 - ri])


def colorize(gray, seed=0):
    """[H,W] grey -> [H,W,3] RGB: R and B a smooth chroma pattern around the grey value, G chosen so that the rule gives back about
    the grey value.  Swapping R and B changes the grey frame, so a wrong channel order shows."""
    h, w = gray.shape
    rng = np.random.default_rng(seed)
    ph = rng.uniform(0, 2 * np.pi, 2)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    g = gray.astype(np.float64)
    r = np.clip(g + 60 * np.sin(2 * np.pi * xx / max(w, 1) * 1.5 + ph[0]), 0, 255).round()
    b = np.clip(g - 60 * np.sin(2 * np.pi * yy / max(h, 1) * 1.2 + ph[1]), 0, 255).round()
    gg = np.clip((g * 16384 - 4899 * r - 1868 * b) / 9617, 0, 255).round()
    return np.stack([r, gg, b], -1).astype(np.uint8)


def undistorted(buf, fmt, w, h, K, dist, pitch=0, offset=0, raw_mask=None):
    """gray -> nmi_undistort_frame, as the twins compute it: (frame, mask)."""
    return unp.undistort(to_gray(buf, fmt, w, h, pitch, offset), K, dist, raw_mask)


def all_triples(start, n):
    """(R, G, B) triples start .. start + n - 1 of the 2^24, R slowest -> [n,3] uint8."""
    i = np.arange(start, start + n, dtype=np.int64)
    return np.stack([(i >> 16) & 255, (i >> 8) & 255, i & 255], -1).astype(np.uint8)
