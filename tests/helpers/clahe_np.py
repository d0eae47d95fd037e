"""numpy restatement of NMI_TONE_CLAHE (include/nmi_hip.h, "Deep frames"): tiled, contrast-limited equalisation of a deep grey
frame -- TEST INFRASTRUCTURE ONLY.

M = 2^bits - 1, L = M + 1, v = min(raw, M); the source is Ws x Hs, cut into tx x ty tiles:
    tiles     column x is in tile column ((2x+1) tx) // (2 Ws), row y in tile row ((2y+1) ty) // (2 Hs)
    table     h_t the tile's exact counts, n_t its pixels, P the plateau.  P == 0: c'' = cumsum(h_t).  P >= 1: E = sum max(h_t - P, 0),
              c' = cumsum(min(h_t, P)), q = E // L, r = E % L, step = max(L // r, 1),
              c''[v] = c'[v] + q (v + 1) + (r ? min(r, v // step + 1) : 0);   T_t[v] = (c''[v] 255 + (n_t >> 1)) // n_t
    blend     ax = (2x+1) tx - Ws, dx = 2 Ws, i0 = ax // dx (floor), wx = ((ax - i0 dx) 256) // dx, i1 = i0 + 1, both clamped to
              0 .. tx-1; j0, j1, wy likewise;  out = ((A (256-wx) + B wx)(256-wy) + (C (256-wx) + D wx) wy + 32768) >> 16
The functions of the first half are the vectorised model (int64) the GPU tests compare with; the naive_* ones restate the rule
with Python loops and cv::CLAHE's loop-form redistribution, only to check the first.  A tone map is tone_np's dict with
"tiles_x" and "tiles_y" added (clahe()).
"""
import numpy as np

from helpers import reduce_np as rnp
from helpers import tone_np as tnp

CLAHE = 6
LEVELS = tnp.LEVELS


def clahe(tiles_x=8, tiles_y=8, plateau=0, bits=16):
    tm = tnp.tone(CLAHE, bits, plateau=plateau)
    tm["tiles_x"], tm["tiles_y"] = tiles_x, tiles_y
    return tm


def capi_tone(capi, tm):
    return capi.ToneMap.clahe(tm["tiles_x"], tm["tiles_y"], tm["plateau"], tm["bits"])


def tile_of(n, tiles):
    """The tile index of each of the n coordinates of an axis."""
    x = np.arange(n, dtype=np.int64)
    return ((2 * x + 1) * tiles) // (2 * n)


def tile_map(ws, hs, tx, ty):
    """[Hs,Ws] the tile (row-major, j * tx + i) of every pixel."""
    return tile_of(hs, ty)[:, None] * tx + tile_of(ws, tx)[None, :]


def tile_histograms(px, bits, tx, ty):
    """[Hs,Ws] uint16 -> int64 [ty*tx, 65536] exact counts of v = min(raw, M) per tile."""
    px = np.asarray(px, np.int64)
    hs, ws = px.shape
    v = np.minimum(px, (1 << bits) - 1)
    key = tile_map(ws, hs, tx, ty) * LEVELS + v
    return np.bincount(key.ravel(), minlength=tx * ty * LEVELS).reshape(ty * tx, LEVELS).astype(np.int64)


def excess(h, plateau, bits):
    """(E, q, r, step) of one tile's counts h; step is 0 where r == 0 (never used)."""
    L = 1 << bits
    if plateau == 0:
        return 0, 0, 0, 0
    e = int(np.maximum(np.asarray(h, np.int64) - plateau, 0).sum())
    r = e % L
    return e, e // L, r, (max(L // r, 1) if r else 0)


def running(h, plateau, bits):
    """c'' of every tile: int64 [tiles, 65536], meaningful for v <= M."""
    h = np.asarray(h, np.int64)
    if plateau == 0:
        return np.cumsum(h, axis=1)
    L = 1 << bits
    e = np.maximum(h - plateau, 0).sum(axis=1)
    c1 = np.cumsum(np.minimum(h, plateau), axis=1)
    q, r = e // L, e % L
    step = np.maximum(L // np.maximum(r, 1), 1)
    v = np.arange(LEVELS, dtype=np.int64)
    extra = np.where(r[:, None] > 0, np.minimum(r[:, None], v[None, :] // step[:, None] + 1), 0)
    return c1 + q[:, None] * (v[None, :] + 1) + extra


def tables_of_histograms(h, bits, plateau):
    """T_t: uint8 [tiles, 65536] (entry i is the value of min(i, M)), and n_t: int64 [tiles]."""
    m = (1 << bits) - 1
    n = np.asarray(h, np.int64).sum(axis=1)
    c2 = running(h, plateau, bits)
    assert (c2[:, m] == n).all()
    t = (c2 * 255 + (n >> 1)[:, None]) // n[:, None]
    t[:, m + 1:] = t[:, m:m + 1]
    assert t.min() >= 0 and t.max() <= 255
    return t.astype(np.uint8), n


def tile_luts(px, tm):
    """nmi_tone_tile_luts of the [Hs,Ws] pixels: (uint8 [ty, tx, 65536], int64 [ty, tx])."""
    tx, ty = tm["tiles_x"], tm["tiles_y"]
    t, n = tables_of_histograms(tile_histograms(px, tm["bits"], tx, ty), tm["bits"], tm["plateau"])
    return t.reshape(ty, tx, LEVELS), n.reshape(ty, tx)


def axis(n, tiles):
    """(lower tile, upper tile, weight of the upper) of each of the n coordinates, tiles clamped to the grid."""
    x = np.arange(n, dtype=np.int64)
    a, d = (2 * x + 1) * tiles - n, 2 * n
    i0 = a // d
    w = ((a - i0 * d) * 256) // d
    assert w.min() >= 0 and w.max() <= 255 and i0.min() >= -1 and i0.max() <= tiles - 1
    return np.clip(i0, 0, tiles - 1), np.clip(i0 + 1, 0, tiles - 1), w


def blend(px, luts, bits):
    """[Hs,Ws] uint16 under the tile tables [ty, tx, 65536] -> [Hs,Ws] uint8."""
    px = np.asarray(px, np.int64)
    hs, ws = px.shape
    ty, tx = luts.shape[:2]
    v = np.minimum(px, (1 << bits) - 1)
    t = np.asarray(luts, np.int64)
    i0, i1, wx = (a[None, :] for a in axis(ws, tx))
    j0, j1, wy = (a[:, None] for a in axis(hs, ty))
    up = t[j0, i0, v] * (256 - wx) + t[j0, i1, v] * wx
    down = t[j1, i0, v] * (256 - wx) + t[j1, i1, v] * wx
    out = (up * (256 - wy) + down * wy + 32768) >> 16
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def apply(px, tm):
    return blend(px, tile_luts(px, tm)[0], tm["bits"])


def to_gray(buf, w, h, tm, pitch=0, offset=0):
    return apply(tnp.pixels(buf, w, h, pitch, offset), tm)


def reduce_frame(buf, w, h, f, tm, pitch=0, offset=0):
    """nmi_reduce_frame on f*h rows of f*w deep pixels: tiles, tables and blend on the full size, then reduce_np's box rule."""
    return rnp.reduce_gray(to_gray(buf, f * w, f * h, tm, pitch, offset), f)


# --- the naive form --------------------------------------------------------------------------------------------------------

def naive_table(values, bits, plateau):
    """One tile's table from the list of its (saturated) pixel values: list of L entries.  cv::CLAHE's loop: clip, hand every
    level E // L, then one more to levels 0, step, 2 step, ... while any of the rest is left."""
    L = 1 << bits
    hist = [0] * L
    for v in values:
        hist[v] += 1
    n = len(values)
    if plateau > 0:
        e = 0
        for i in range(L):
            if hist[i] > plateau:
                e += hist[i] - plateau
                hist[i] = plateau
        batch, rest = e // L, e % L
        for i in range(L):
            hist[i] += batch
        if rest:
            step = max(L // rest, 1)
            i = 0
            while i < L and rest > 0:
                hist[i] += 1
                i += step
                rest -= 1
    out, c = [], 0
    for i in range(L):
        c += hist[i]
        out.append((c * 255 + (n >> 1)) // n)
    assert c == n
    return out


def naive_apply(px, tm):
    """[Hs,Ws] -> ([Hs,Ws] uint8, tables [ty][tx] of L entries, counts [ty][tx]) by loops over pixels."""
    bits, tx, ty, plateau = tm["bits"], tm["tiles_x"], tm["tiles_y"], tm["plateau"]
    m = (1 << bits) - 1
    hs, ws = len(px), len(px[0])
    members = [[[] for _ in range(tx)] for _ in range(ty)]
    for y in range(hs):
        for x in range(ws):
            members[((2 * y + 1) * ty) // (2 * hs)][((2 * x + 1) * tx) // (2 * ws)].append(min(int(px[y][x]), m))
    tables = [[naive_table(members[j][i], bits, plateau) for i in range(tx)] for j in range(ty)]
    counts = [[len(members[j][i]) for i in range(tx)] for j in range(ty)]

    def where(c, tiles, size):
        a, d = (2 * c + 1) * tiles - size, 2 * size
        k = a // d                                   # (Python's // floors)
        return min(max(k, 0), tiles - 1), min(max(k + 1, 0), tiles - 1), ((a - k * d) * 256) // d

    out = np.zeros((hs, ws), np.uint8)
    for y in range(hs):
        j0, j1, wy = where(y, ty, hs)
        for x in range(ws):
            i0, i1, wx = where(x, tx, ws)
            v = min(int(px[y][x]), m)
            up = tables[j0][i0][v] * (256 - wx) + tables[j0][i1][v] * wx
            down = tables[j1][i0][v] * (256 - wx) + tables[j1][i1][v] * wx
            out[y, x] = (up * (256 - wy) + down * wy + 32768) >> 16
    return out, tables, counts


# --- contents --------------------------------------------------------------------------------------------------------------

def tile_box(ws, hs, tx, ty, i, j):
    """(x0, x1, y0, y1) of tile (i, j)."""
    cx, cy = np.flatnonzero(tile_of(ws, tx) == i), np.flatnonzero(tile_of(hs, ty) == j)
    return int(cx[0]), int(cx[-1]) + 1, int(cy[0]), int(cy[-1]) + 1


def plant_distinct(px, bits, tx, ty, i, j, distinct, seed=0):
    """A copy of px whose tile (i, j) holds exactly `distinct` different values below 2^bits: one of them on every pixel to
    spare, the others once each.  With plateau 1 the tile's excess is then n_t - distinct.  Returns (frame, the heavy value's count)."""
    out = np.array(px, np.uint16)
    hs, ws = out.shape
    x0, x1, y0, y1 = tile_box(ws, hs, tx, ty, i, j)
    n = (x1 - x0) * (y1 - y0)
    assert 1 <= distinct <= min(n, 1 << bits)
    rng = np.random.default_rng(seed)
    levels = rng.choice(1 << bits, size=distinct, replace=False)
    vals = np.full(n, levels[0])
    vals[:distinct - 1] = levels[1:]
    out[y0:y1, x0:x1] = rng.permutation(vals).reshape(y1 - y0, x1 - x0)
    return out, n - distinct + 1


def halves(w, h, left=1000, right=40000, spread=200, seed=0):
    """A left half near `left`, a right half near `right`: tiles whose tables differ strongly."""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, spread, (h, w)) + np.where(np.arange(w)[None, :] < w // 2, left, right)
    return img.astype(np.uint16)
