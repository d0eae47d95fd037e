"""The sizes and planted frames of the deep intake's launch-geometry tests (tests/test_packed_seams.py, tests/test_valid_seams.py
and the second-trip cases of tests/test_clahe_tables.py) -- TEST INFRASTRUCTURE ONLY.  tests/test_intake_geometry.py proves on
the CPU, through helpers/intake_geometry.py, that every size reaches the branch it is here for."""
import functools

import numpy as np

from helpers import intake_geometry as geo
from helpers import packed_np as pnp
from helpers import valid_cases
from helpers import valid_np as vnp

# --- nmi_unpack_frame -----------------------------------------------------------------------------------------------------------------
# Source widths (context = width, factor 1): below one run, every tail the layout allows, two and three block columns.
UNPACK_WIDTHS = {
    pnp.GRAY16_BE: (1, 3, 5, 7, 9, 513, 514, 516, 518, 520, 1031),
    pnp.MONO10P: (4, 12, 516, 520, 1028),
    pnp.RAW10: (4, 12, 516, 520, 1028),
    pnp.MONO12P: (2, 6, 10, 14, 514, 516, 518, 520, 1030),
    pnp.RAW12: (2, 6, 10, 14, 514, 516, 518, 520, 1030),
}
UNPACK_HEIGHTS = (1, 5)
UNPACK_TAILS = {pnp.GRAY16_BE: {1, 2, 3, 4, 5, 6, 7, 8}, pnp.MONO10P: {4, 8}, pnp.RAW10: {4, 8}, pnp.MONO12P: {2, 4, 6, 8},
                pnp.RAW12: {2, 4, 6, 8}}
UNPACK_FACTOR3 = (172, 2)                  # context; its factor-3 source is 516 x 6
# the container's base, bytes past a 16-byte boundary, and the widths it is swept at: 520 takes vec 2 / 1 / 0 by the base alone,
# 516 vec 1 / 0, 518 vec 0 whatever the base
OUT_BASES = (0, 2, 8, 10)
OUT_WIDTHS = (520, 516, 518)
OUT_HEIGHT = 5
BAYER_SIZES = ((513, 5), (514, 2), (519, 3), (520, 5), (1031, 5))
BAYER_OUT_SIZE = (520, 5)
CHAIN_SIZE = (520, 8)


def out_widths(fmt):
    return tuple(w for w in OUT_WIDTHS if pnp.row_bytes(fmt, w) > 0)


# --- the valid-range conversions ------------------------------------------------------------------------------------------------------
# 264 x 8: whole quads, two block columns; 261 x 9: the last quad holds one pixel, byte stores.  (8 rows: the 8 x 8 CLAHE grid.)
VALID_SIZES = [(264, 8), (261, 9)]
VALID_FRAMES = ("depth_holes", "dead_pixels", "tail_pixel", "wide_holes", "seam_pixels")
SEAM = 256                                 # the first output column of block column 1


def seam_columns(w):
    return (SEAM - 1, SEAM, w - 1)


def valid_frame(name, w, h, f, seed=1):
    """valid_cases.frame, and the plant of this file: (pixels [f*h, f*w] uint16, range, bits)."""
    if name == "seam_pixels":
        return vnp.seam_pixels(f * w, f * h, f, seam_columns(w), seed)[:3]
    return valid_cases.frame(name, w, h, f, seed)


# --- second trips of the histogram loops ----------------------------------------------------------------------------------------------
# (context W, H, factor): one source of 2104 x 2012 pixels at factor 4, one of 2101 x 2011 at factor 1
SECOND_TRIP_RUNS = {"f4": (526, 503, 4), "f1": (2101, 2011, 1)}
SECOND_TRIP_GRID = (8, 8)
LATE_RANGE = (1, 65534)
LATE_FLOOR = (1 << 15) + (1 << 14)


def late_quarters(trip, seed=0):
    """[Hs,Ws] uint16 from the map `trip` of the loop trip on which a histogram kernel loads each pixel: every pixel of a first
    trip below 2^15, every pixel only a later trip reads at 2^15 + 2^14 or above; about one early pixel in 500 is 0 and about one
    late pixel in 50 is 65535, both invalid under LATE_RANGE."""
    rng = np.random.default_rng(seed)
    late = np.asarray(trip) > 0
    px = np.where(late, rng.integers(LATE_FLOOR, 65535, late.shape), rng.integers(1, 1 << 15, late.shape))
    px[~late & (rng.random(late.shape) < 0.002)] = 0
    px[late & (rng.random(late.shape) < 0.02)] = 65535
    return px.astype(np.uint16)


@functools.lru_cache(maxsize=None)
def second_trip_frame(run, kernel):
    """The late_quarters frame of SECOND_TRIP_RUNS[run] for `kernel`: "tone" (row-major runs of the whole frame) or "clahe" (the
    tile-local numbering of the 8 x 8 grid).  Cached and read-only: the tests share it."""
    w, h, f = SECOND_TRIP_RUNS[run]
    ws, hs = f * w, f * h
    if kernel == "tone":
        trip = geo.tone_hist_trip_map(ws, hs)
    else:
        trip = geo.clahe_trip_map(*SECOND_TRIP_GRID, ws, hs)
    px = late_quarters(trip, seed=len(run) + len(kernel) + f)
    px.setflags(write=False)
    return px
