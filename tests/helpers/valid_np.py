"""numpy restatement of the valid range of deep grey frames (nmi_set_valid_range, include/nmi_hip.h "Deep frames") -- TEST
INFRASTRUCTURE ONLY.

A range is a pair (lo, hi), 0 <= lo <= hi <= 65535; OFF = (0, 65535).  A source pixel is valid iff lo <= raw <= hi, raw being the
16-bit container's value before it saturates to M = 2^bits - 1:
    statistics   h[v] counts the valid pixels only and N is their number (CLAHE: h_t, n_t per tile); the tables are tone_np's and
                 clahe_np's of those counts
    no pixels    a global mode with N == 0: the table all 0, the window (0, 0); a CLAHE tile with n_t == 0: SHIFT's table
    grey bytes   every pixel, valid or not, goes through the table (CLAHE: the blend) as before
    mask         [H,W] uint8 at the search size: 1 iff all f x f source pixels are valid (reduce_np.reduce_mask) and the frame
                 mask's byte, where one is given, is nonzero
The tables come from tone_np.table and clahe_np.tables_of_histograms, which this file only calls.
"""
import numpy as np

from helpers import clahe_np as cnp
from helpers import reduce_np as rnp
from helpers import tone_np as tnp

OFF = (0, 65535)
LEVELS = tnp.LEVELS


def is_on(rng):
    return tuple(rng) != OFF


def tiled(tm):
    return tm["mode"] == cnp.CLAHE


def from_frame(tm):
    return tm["mode"] in (tnp.PERCENTILE, tnp.EQUALIZE, cnp.CLAHE)


def valid(px, rng):
    """[Hs,Ws] uint16 -> bool: lo <= raw <= hi."""
    px = np.asarray(px, np.int64)
    return (px >= rng[0]) & (px <= rng[1])


def histogram(px, bits, rng):
    """int64 [65536] counts of v = min(raw, M) over the valid pixels."""
    px = np.asarray(px, np.int64)
    v = np.minimum(px, (1 << bits) - 1)[valid(px, rng)]
    return np.bincount(v.ravel(), minlength=LEVELS).astype(np.int64)


def table_of_histogram(tm, h):
    """tone_np.table, and the N == 0 rule for the modes that read h."""
    if tm["mode"] in (tnp.PERCENTILE, tnp.EQUALIZE) and int(np.asarray(h).sum()) == 0:
        return np.zeros(LEVELS, np.uint8), (0, 0)
    return tnp.table(tm, h)


def table(px, tm, rng):
    """nmi_tone_lut's (table, (lo, hi)) of the [Hs,Ws] pixels under the range."""
    return table_of_histogram(tm, histogram(px, tm["bits"], rng) if tm["mode"] in (tnp.PERCENTILE, tnp.EQUALIZE) else None)


def tile_histograms(px, bits, tx, ty, rng):
    """int64 [ty*tx, 65536] counts of v = min(raw, M) over each tile's valid pixels."""
    px = np.asarray(px, np.int64)
    hs, ws = px.shape
    ok = valid(px, rng)
    key = (cnp.tile_map(ws, hs, tx, ty) * LEVELS + np.minimum(px, (1 << bits) - 1))[ok]
    return np.bincount(key.ravel(), minlength=tx * ty * LEVELS).reshape(ty * tx, LEVELS).astype(np.int64)


def shift_table(bits):
    return tnp.table(tnp.tone(tnp.SHIFT, bits))[0]


def tables_of_tile_histograms(h, bits, plateau):
    """clahe_np.tables_of_histograms for the tiles that hold a pixel, SHIFT's table for those that hold none."""
    h = np.asarray(h, np.int64)
    n = h.sum(axis=1)
    t = np.empty((h.shape[0], LEVELS), np.uint8)
    full = n > 0
    if full.any():
        t[full], n_full = cnp.tables_of_histograms(h[full], bits, plateau)
        assert (n_full == n[full]).all()
    t[~full] = shift_table(bits)
    return t, n


def tile_luts(px, tm, rng):
    """nmi_tone_tile_luts under the range: (uint8 [ty, tx, 65536], int64 [ty, tx] valid pixels per tile)."""
    tx, ty = tm["tiles_x"], tm["tiles_y"]
    t, n = tables_of_tile_histograms(tile_histograms(px, tm["bits"], tx, ty, rng), tm["bits"], tm["plateau"])
    return t.reshape(ty, tx, LEVELS), n.reshape(ty, tx)


def apply(px, tm, rng):
    """[Hs,Ws] uint16 -> [Hs,Ws] uint8: every pixel through the tables of the valid ones."""
    if tiled(tm):
        return cnp.blend(px, tile_luts(px, tm, rng)[0], tm["bits"])
    return table(px, tm, rng)[0][np.asarray(px, np.int64)]


def mask(px, f, rng, frame_mask=None):
    """[f*H, f*W] uint16 -> the validity mask [H,W] uint8, ANDed with frame_mask ([H,W], nonzero = usable) where given."""
    m = rnp.reduce_mask(valid(px, rng), f)
    if frame_mask is not None:
        m = m & (np.asarray(frame_mask) != 0).astype(np.uint8)
    return m


def deep_frame(px, f, tm, rng, frame_mask=None):
    """nmi_deep_frame of the full-size pixels [f*H, f*W]: (grey [H,W], mask [H,W])."""
    return rnp.reduce_gray(apply(px, tm, rng), f), mask(px, f, rng, frame_mask)


def float_tables(px, tm, rng):
    """The quotients of EQUALIZE and CLAHE in float64, from the valid pixels listed one by one: uint8 [65536] (EQUALIZE) or
    [ty, tx, 65536] (CLAHE, plateau 0).  A second way to the same tables."""
    bits = tm["bits"]
    m = (1 << bits) - 1
    px = np.asarray(px, np.int64)
    ok = valid(px, rng)
    v_all = np.minimum(np.arange(LEVELS), m)

    def counts_below(values):   # c[v] = #(values <= v), by sorting instead of a histogram
        return np.searchsorted(np.sort(values), v_all, side="right").astype(np.float64)

    if tm["mode"] == tnp.EQUALIZE:
        assert tm["plateau"] == 0
        vals = np.minimum(px, m)[ok]
        if vals.size == 0:
            return np.zeros(LEVELS, np.uint8)
        c = counts_below(vals)
        vmin = int(vals.min())
        c0 = float((vals == vmin).sum())
        den = float(vals.size) - c0
        if den == 0:
            return np.zeros(LEVELS, np.uint8)
        out = np.where(v_all >= vmin, np.floor(((c - c0) * 255.0 + float(int(den) >> 1)) / den), 0.0)
        return out.astype(np.uint8)
    assert tiled(tm) and tm["plateau"] == 0
    tx, ty = tm["tiles_x"], tm["tiles_y"]
    tiles = cnp.tile_map(px.shape[1], px.shape[0], tx, ty)
    out = np.empty((ty * tx, LEVELS), np.uint8)
    for t in range(tx * ty):
        vals = np.minimum(px, m)[ok & (tiles == t)]
        if vals.size == 0:
            out[t] = v_all >> (bits - 8)
            continue
        n = float(vals.size)
        out[t] = np.floor((counts_below(vals) * 255.0 + float(vals.size >> 1)) / n).astype(np.uint8)
    return out.reshape(ty, tx, LEVELS)


# --- contents: frames with planted sentinels ------------------------------------------------------------------------------------
# Each returns (pixels [Hs,Ws] uint16, range, bits).  tests/test_valid_twin.py checks on every one of them that the ranged table
# differs from the unranged one and that the mask is neither all 0 nor all 1.

def depth_holes(ws, hs, share=0.3, seed=0):
    """A depth frame, 500 .. 9000 mm in 14 bits, with `share` of its pixels 0 (no return): range (1, 65535)."""
    rng = np.random.default_rng(seed)
    px = rng.integers(500, 9001, (hs, ws))
    px[rng.random((hs, ws)) < share] = 0
    return px.astype(np.uint16), (1, 65535), 14


def dead_pixels(ws, hs, count=5, seed=0):
    """A 12-bit scene 100 .. 3000 in a 16-bit container with `count` dead pixels at 65535: range (0, 4095).  Unranged, the
    sentinels count as 4095."""
    rng = np.random.default_rng(seed)
    px = rng.integers(100, 3001, (hs, ws))
    px.reshape(-1)[rng.choice(ws * hs, size=count, replace=False)] = 65535
    return px.astype(np.uint16), (0, 4095), 12


def lone_sentinel(ws, hs, seed=0):
    """Bits 16, every pixel below 2^14 but one 65535 (not in a corner block): range (0, 65534).  With the range the frame is a
    one-pass frame for the histogram, and a min-max stretch is not all black."""
    rng = np.random.default_rng(seed)
    px = rng.integers(2000, 12000, (hs, ws))
    px[hs // 2, ws // 2] = 65535
    return px.astype(np.uint16), (0, 65534), 16


def tail_pixel(ws, hs, f=1, seed=0):
    """An invalid pixel (0) under the last output pixel of the last row -- the partial tail quad where W % 4 != 0 -- and one under
    output pixel (0, 0): range (1, 65535), 14 bits."""
    rng = np.random.default_rng(seed)
    px = rng.integers(3000, 16000, (hs, ws))
    px[hs - 1, ws - 1] = 0
    px[0, 0] = 0
    return px.astype(np.uint16), (1, 65535), 14


def block_corner(ws, hs, f, seed=0):
    """Invalid pixels (65535) in one corner each of a few f x f blocks, a different corner per block: range (0, 16383), 14 bits."""
    rng = np.random.default_rng(seed)
    px = rng.integers(0, 16384, (hs, ws))
    w, h = ws // f, hs // f
    corners = [(0, 0), (0, f - 1), (f - 1, 0), (f - 1, f - 1)]
    for i, (dy, dx) in enumerate(corners):
        bx, by = (3 + 5 * i) % w, (2 + 3 * i) % h
        px[by * f + dy, bx * f + dx] = 65535
    return px.astype(np.uint16), (0, 16383), 14


def seam_pixels(ws, hs, f, columns, seed=0):
    """Exactly one invalid source pixel (0) in the f x f block of one output pixel per entry of `columns` (output x), each on a
    different output row and in a different corner of its block; everything else valid: range (1, 65535), 14 bits.  Returns
    (pixels, range, bits, [(x, y) of the output pixels whose mask is 0])."""
    rng = np.random.default_rng(seed)
    px = rng.integers(3000, 16000, (hs, ws))
    h = hs // f
    assert len(columns) <= min(h, 4)
    corners = [(f - 1, f - 1), (0, f - 1), (f - 1, 0), (0, 0)]                  # (dy, dx)
    rows = [(1 + i * (h - 2) // max(len(columns) - 1, 1)) for i in range(len(columns))]   # from row 1 to the last row
    assert len(set(rows)) == len(rows) and max(rows) == h - 1
    for x, y, (dy, dx) in zip(columns, rows, corners):
        px[y * f + dy, x * f + dx] = 0
    return px.astype(np.uint16), (1, 65535), 14, list(zip(columns, rows))


def nothing_valid(ws, hs, seed=0):
    """Every pixel outside the range (100, 200): N == 0.  (The one content whose mask is all 0.)"""
    rng = np.random.default_rng(seed)
    return rng.integers(1000, 60000, (hs, ws)).astype(np.uint16), (100, 200), 16


def empty_tile(ws, hs, tx, ty, i=0, j=0, seed=0):
    """halves-like content whose tile (i, j) is all 0 (a wholly invalid tile beside valid ones): range (1, 65535), 16 bits."""
    px = cnp.halves(ws, hs, left=1200, right=41000, seed=seed)
    x0, x1, y0, y1 = cnp.tile_box(ws, hs, tx, ty, i, j)
    px[y0:y1, x0:x1] = 0
    return px, (1, 65535), 16
