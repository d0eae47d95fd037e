"""numpy restatement of the deep grey frames of nmi_gray_frame (NMI_FRAME_GRAY16, include/nmi_hip.h "Deep frames") -- TEST
INFRASTRUCTURE ONLY.

A tone map turns the 16-bit container's pixels into 8 bits through one table of 65,536 entries, all in integers.  M = 2^bits - 1,
v = min(raw, M), N = the pixels covered, h[v] their exact counts, c[v] the inclusive running sum:
    SHIFT       v >> (bits - 8)
    WINDOW      v <= lo: 0; else v >= hi: 255; else ((v - lo) * 255 + ((hi - lo) >> 1)) // (hi - lo)
    PERCENTILE  lo = min v with c[v] > N * p_lo // 10000, hi = min v with c[v] >= N - N * p_hi // 10000, then WINDOW
    EQUALIZE    h' = min(h, plateau) (plateau 0: h), c' its running sum, T = c'[M], c0 = h'[vmin]:
                T == c0: 0; else v < vmin: 0, else ((c'[v] - c0) * 255 + ((T - c0) >> 1)) // (T - c0)
    TABLE       lut[v]
A tone map here is a dict: {"mode": ..., "bits": ..., and the mode's fields}; tone(...) builds one.  pack16() lays a frame out
with noise in every byte the rule must not read; to_gray() and reduce_frame() are the rule on such a buffer.
"""
import numpy as np

from helpers import reduce_np as rnp

GRAY16 = 48
SHIFT, WINDOW, PERCENTILE, EQUALIZE, TABLE = 0, 1, 2, 3, 4
LEVELS = 65536


def tone(mode=SHIFT, bits=16, lo=0, hi=0, p_lo=0, p_hi=0, plateau=0, lut=None):
    return {"mode": mode, "bits": bits, "lo": lo, "hi": hi, "p_lo": p_lo, "p_hi": p_hi, "plateau": plateau, "lut": lut}


def histogram(px, bits):
    """[H,W] uint16 pixels -> int64 [65536] counts of v = min(raw, M)."""
    m = (1 << bits) - 1
    return np.bincount(np.minimum(np.asarray(px, np.int64), m).ravel(), minlength=LEVELS).astype(np.int64)


def window_rule(v, lo, hi):
    v = np.asarray(v, np.int64)
    span = max(hi - lo, 1)
    mid = ((v - lo) * 255 + ((hi - lo) >> 1)) // span
    return np.where(v <= lo, 0, np.where(v >= hi, 255, mid)).astype(np.int64)


def percentile_pair(h, p_lo, p_hi):
    c = np.cumsum(h)
    n = int(c[-1])
    k_lo, k_hi = n * p_lo // 10000, n * p_hi // 10000
    return int(np.argmax(c > k_lo)), int(np.argmax(c >= n - k_hi))


def table(tm, h=None):
    """The tone map's table, uint8 [65536] (entry i is the value of v = min(i, M)), and the {lo, hi} pair nmi_tone_lut reports.
    h: the frame's histogram (PERCENTILE, EQUALIZE)."""
    bits, mode = tm["bits"], tm["mode"]
    m = (1 << bits) - 1
    v = np.minimum(np.arange(LEVELS, dtype=np.int64), m)
    pair = (0, m)
    if mode == SHIFT:
        out = v >> (bits - 8)
    elif mode == WINDOW:
        pair = (tm["lo"], tm["hi"])
        out = window_rule(v, *pair)
    elif mode == PERCENTILE:
        pair = percentile_pair(h, tm["p_lo"], tm["p_hi"])
        out = window_rule(v, *pair)
    elif mode == EQUALIZE:
        present = np.flatnonzero(h)
        vmin, vmax = int(present[0]), int(present[-1])
        pair = (vmin, vmax)
        hc = np.minimum(h, tm["plateau"]) if tm["plateau"] else h
        c = np.cumsum(hc)
        t, c0 = int(c[m]), int(hc[vmin])
        if t == c0:
            out = np.zeros(LEVELS, np.int64)
        else:
            out = np.where(v >= vmin, ((c[v] - c0) * 255 + ((t - c0) >> 1)) // (t - c0), 0)
    elif mode == TABLE:
        out = np.asarray(tm["lut"], np.int64)[v]
    else:
        raise ValueError(mode)
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8), pair


def row_bytes(w, pitch=0):
    return pitch if pitch else 2 * w


def span(w, h, pitch=0):
    return (h - 1) * row_bytes(w, pitch) + 2 * w


def pack16(img, pitch=0, offset=0, seed=0):
    """img: [H,W] uint16 -> flat uint8 buffer: `offset` noise bytes, then the H rows of `pitch` bytes, little-endian; the offset
    and the pitch's padding hold noise."""
    img = np.asarray(img, np.uint16)
    h, w = img.shape
    rb = row_bytes(w, pitch)
    rng = np.random.default_rng(seed)
    buf = rng.integers(0, 256, offset + (h - 1) * rb + 2 * w, dtype=np.uint8)
    le = img.astype("<u2").view(np.uint8).reshape(h, 2 * w)
    for y in range(h):
        buf[offset + y * rb:offset + y * rb + 2 * w] = le[y]
    return buf


def pixels(buf, w, h, pitch=0, offset=0):
    """The [H,W] uint16 pixels of a flat buffer laid out as pack16() lays it out."""
    rb = row_bytes(w, pitch)
    buf = np.asarray(buf, np.uint8)
    rows = np.stack([buf[offset + y * rb:offset + y * rb + 2 * w] for y in range(h)])
    return (rows[:, 0::2].astype(np.uint16) | (rows[:, 1::2].astype(np.uint16) << 8))


def apply(px, tm):
    """[H,W] uint16 -> [H,W] uint8 under the tone map, its statistics taken from px itself."""
    lut, _ = table(tm, histogram(px, tm["bits"]) if tm["mode"] in (PERCENTILE, EQUALIZE) else None)
    return lut[np.asarray(px, np.int64)]


def to_gray(buf, w, h, tm, pitch=0, offset=0):
    return apply(pixels(buf, w, h, pitch, offset), tm)


def reduce_frame(buf, w, h, f, tm, pitch=0, offset=0):
    """nmi_reduce_frame on f*h rows of f*w deep pixels -> [h,w] uint8: the full-size frame's statistics, each source pixel mapped,
    then reduce_np's box rule."""
    return rnp.reduce_gray(to_gray(buf, f * w, f * h, tm, pitch, offset), f)


def lut_of(buf, w, h, tm, pitch=0, offset=0):
    """nmi_tone_lut's (table, (lo, hi)) for the frame in buf."""
    px = pixels(buf, w, h, pitch, offset)
    return table(tm, histogram(px, tm["bits"]) if tm["mode"] in (PERCENTILE, EQUALIZE) else None)


# --- contents --------------------------------------------------------------------------------------------------------------

def uniform(w, h, seed=0):
    return np.random.default_rng(seed).integers(0, 65536, (h, w)).astype(np.uint16)


def flat(w, h, value=7123):
    return np.full((h, w), value, np.uint16)


def two_valued(w, h, a=1000, b=40000, seed=0):
    return np.where(np.random.default_rng(seed).random((h, w)) < 0.3, a, b).astype(np.uint16)


def thermal(w, h, seed=0):
    """A 14-bit band 7000 .. 7400 with (up to) twenty pixels at 16383."""
    rng = np.random.default_rng(seed)
    img = rng.integers(7000, 7401, (h, w)).astype(np.uint16)
    hot = rng.choice(w * h, size=min(20, w * h // 2), replace=False)
    img.reshape(-1)[hot] = 16383
    return img


def over_depth(w, h, seed=0):
    """For bits = 12: half the pixels inside 0 .. 4095, half anywhere up to 65535."""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 4096, (h, w))
    wide = rng.integers(0, 65536, (h, w))
    return np.where(rng.random((h, w)) < 0.5, img, wide).astype(np.uint16)


def planted(w, h, count, value=30000, seed=0):
    """`value` exactly `count` times, the other pixels spread over the other values."""
    rng = np.random.default_rng(seed)
    n = w * h
    assert count <= n
    rest = rng.integers(0, 65535, n)
    rest[rest >= value] += 1
    flat_img = rest.astype(np.uint16)
    flat_img[rng.choice(n, size=count, replace=False)] = value
    assert int((flat_img == value).sum()) == count
    return flat_img.reshape(h, w)


def capi_tone(capi, tm, d_lut=None):
    """The tone map as the binding's ToneMap (orbslam2_nmi_amd.capi); d_lut: the device tensor of a TABLE's lut."""
    mode = tm["mode"]
    if mode == TABLE:
        return capi.ToneMap.from_table(d_lut, tm["bits"])
    return capi.ToneMap(mode=mode, bits=tm["bits"], lo=tm["lo"], hi=tm["hi"], p_lo=tm["p_lo"], p_hi=tm["p_hi"], plateau=tm["plateau"])
