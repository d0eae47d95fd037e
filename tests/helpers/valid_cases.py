"""The cases the valid-range tests share (tests/test_valid_*.py): sizes, planted frames, tone maps, buffer layouts -- TEST
INFRASTRUCTURE ONLY.  The frames are valid_np's; tests/test_valid_twin.py checks their premises on the CPU."""
import numpy as np

from helpers import clahe_np as cnp
from helpers import tone_np as tnp
from helpers import valid_np as vnp

# 40 x 24: whole quads and runs; 37 x 23: the conversion's last quad and the histogram's last run of a row are partial
SIZES = [(40, 24), (37, 23)]
FACTORS = (1, 2, 3, 4)

# name -> how frame() builds it.  bits: the depth the frame is read at (12 and 14 take one histogram pass, 16 four -- one where
# the range leaves nothing above 14 bits).  same_under: labels of tone_maps() whose table the range legitimately leaves alone.
FRAMES = {
    "depth_holes": {"factors": FACTORS, "same_under": ()},
    "dead_pixels": {"factors": FACTORS, "same_under": ()},
    "lone_sentinel": {"factors": FACTORS, "same_under": ("percentile",)},     # one pixel of thousands: inside the 1 % cut
    "tail_pixel": {"factors": FACTORS, "same_under": ()},
    "block_corner": {"factors": FACTORS, "same_under": ()},
    "nothing_valid": {"factors": FACTORS, "same_under": ()},
    "empty_tile": {"factors": FACTORS, "same_under": ()},
    "wide_holes": {"factors": FACTORS, "same_under": ()},
}


def frame(name, w, h, f, seed=1):
    """(pixels [f*h, f*w] uint16, range, bits) of the planted frame `name` for a w x h context at factor f."""
    ws, hs = f * w, f * h
    if name == "depth_holes":
        return vnp.depth_holes(ws, hs, 0.3, seed)
    if name == "dead_pixels":
        return vnp.dead_pixels(ws, hs, max(5, ws * hs // 30), seed)
    if name == "lone_sentinel":
        return vnp.lone_sentinel(ws, hs, seed)
    if name == "tail_pixel":                                 # 5 % holes, and the two forced ones
        px, rng, bits = vnp.tail_pixel(ws, hs, f, seed)
        px[np.random.default_rng(seed + 1).random((hs, ws)) < 0.05] = 0
        px[hs - 1, ws - 1] = px[0, 0] = 0
        px[hs - 1, ws - 2 * f:ws - f] = 5000                 # the output pixel before the tail one stays valid
        px[hs - f:hs - 1, ws - 2 * f:ws - f] = 5000
        return px, rng, bits
    if name == "block_corner":
        return vnp.block_corner(ws, hs, f, seed)
    if name == "nothing_valid":
        return vnp.nothing_valid(ws, hs, seed)
    if name == "empty_tile":                                 # tile (1, 0) of the 3 x 2 grid (and what of the 8 x 8 grid lies in it)
        return vnp.empty_tile(ws, hs, 3, 2, 1, 0, seed)
    if name == "wide_holes":                                 # all 16 bits in use (four histogram passes) with 0-holes
        px = tnp.uniform(ws, hs, seed)
        px[np.random.default_rng(seed + 2).random((hs, ws)) < 0.2] = 0
        return px, (1, 65535), 16
    raise KeyError(name)


def tone_maps(bits, ws=None, hs=None):
    """Every mode, and CLAHE at 1 x 1, 3 x 2 and 8 x 8 tiles: a list of tone_np / clahe_np dicts with a "label"."""
    m = (1 << bits) - 1
    lut = np.random.default_rng(bits).integers(0, 256, 65536).astype(np.uint8)
    maps = [("shift", tnp.tone(tnp.SHIFT, bits)), ("window", tnp.tone(tnp.WINDOW, bits, lo=m // 16, hi=m // 2)),
            ("percentile", tnp.tone(tnp.PERCENTILE, bits, p_lo=100, p_hi=100)), ("minmax", tnp.tone(tnp.PERCENTILE, bits)),
            ("equalize", tnp.tone(tnp.EQUALIZE, bits)), ("plateau", tnp.tone(tnp.EQUALIZE, bits, plateau=2)),
            ("table", tnp.tone(tnp.TABLE, bits, lut=lut)),
            ("clahe1x1", cnp.clahe(1, 1, 0, bits)), ("clahe3x2", cnp.clahe(3, 2, 2, bits)), ("clahe8x8", cnp.clahe(8, 8, 1, bits))]
    out = []
    for label, tm in maps:
        tm = dict(tm)
        tm["label"] = label
        out.append(tm)
    return out


# (pitch beyond the dense row in bytes, offset of the base in bytes): dense and 16-byte aligned; pitched with spare bytes; a base
# 2 bytes off 16-byte alignment -- the last two turn the histogram's and the conversion's vector loads off
LAYOUTS = [(0, 0), (6, 0), (0, 2)]


def layout(ws, extra, off):
    return (2 * ws + extra if extra else 0), off


def capi_tone(capi, tm, d_lut=None):
    return cnp.capi_tone(capi, tm) if vnp.tiled(tm) else tnp.capi_tone(capi, tm, d_lut)
