"""numpy restatement of the full-size frame reduction (nmi_reduce_frame, include/nmi_hip.h) -- TEST INFRASTRUCTURE ONLY.

A source of f * H rows of f * W pixels in an NMI_FRAME_* format is turned grey pixel by pixel (helpers/color_np.py: to_gray), and
output pixel (x, y) is the rounded box average of the f x f grey values at (f x .., f y ..).  round_sum() is the integer rule per
factor, float_form() the float32 form it restates (f = 3, 4: rint(fl32(s) * fl32(1 / f^2)); f = 2: halves rounded up).
reduce_mask() is the mask rule: 1 where a whole block is nonzero.
"""
import numpy as np

from helpers import color_np as cnp

FACTORS = (1, 2, 3, 4)


def round_sum(s, f):
    """The integer sum s of f * f grey values -> their rounded mean (uint8)."""
    s = np.asarray(s, np.int64)
    if f == 1:
        out = s
    elif f == 2:
        out = (s + 2) >> 2
    elif f == 3:
        out = (s + 4) // 9
    elif f == 4:
        q, r = s >> 4, s & 15
        out = q + ((r > 8) | ((r == 8) & ((q & 1) == 1)))
    else:
        raise ValueError(f"factor {f}")
    return out.astype(np.uint8)


def float_form(s, f):
    """The float32 form the integer rule restates.  f = 3, 4: rint(fl32(s) * fl32(1 / f^2)), round half to even.  f = 2: the 2x2
    fast path rounds halves up, floor(fl32(s) * 0.25 + 0.5) (every value here is exact in float32)."""
    x = np.asarray(s).astype(np.float32)
    if f == 2:
        return np.floor(x * np.float32(0.25) + np.float32(0.5)).astype(np.int64)
    scale = np.float32(1.0) / np.float32(f * f)
    return np.rint(x * scale).astype(np.int64)


def block_sums(gray, f):
    """[f*H, f*W] uint8 -> [H, W] int64 sums of the f x f blocks."""
    fh, fw = gray.shape
    h, w = fh // f, fw // f
    return gray[:h * f, :w * f].astype(np.int64).reshape(h, f, w, f).sum(axis=(1, 3))


def reduce_gray(gray, f):
    """A dense grey frame [f*H, f*W] -> [H, W] uint8."""
    return round_sum(block_sums(gray, f), f)


def reduce_frame(buf, fmt, w, h, f, pitch=0, offset=0):
    """The rule on a flat buffer laid out as color_np.pack() lays out a frame of f*h rows of f*w pixels -> [h, w] uint8.  (w, h)
    is the output's size; a pitch wider than f*w pixels crops spare columns, rows beyond f*h are not read."""
    return reduce_gray(cnp.to_gray(buf, fmt, f * w, f * h, pitch, offset), f)


def reduce_mask(mask, f):
    """[f*H, f*W] uint8 / bool -> [H, W] uint8: 1 where all f x f bytes are nonzero."""
    nz = (np.asarray(mask) != 0).astype(np.uint8)
    return (block_sums(nz, f) == f * f).astype(np.uint8)


def every_sum_frame(f, w, h, seed=0):
    """A grey frame [f*h, f*w] in whose f x f blocks every sum 0 .. 255 * f * f occurs (block k has sum k mod (255 f^2 + 1), its
    parts spread at random over the block's pixels).  Needs w * h >= 255 f^2 + 1."""
    n = 255 * f * f + 1
    assert w * h >= n
    rng = np.random.default_rng(seed)
    sums = np.arange(w * h) % n
    # fill the f*f cells of each block in a random order, each taking min(255, what is left)
    cells = np.zeros((w * h, f * f), np.int64)
    left = sums.copy()
    for c in range(f * f):
        cap = np.minimum(255, left)
        # leave enough room in the remaining cells: at least left - 255 * (cells after this one)
        low = np.maximum(0, left - 255 * (f * f - 1 - c))
        take = rng.integers(low, cap + 1)
        cells[:, c] = take
        left -= take
    assert (left == 0).all()
    perm = rng.permuted(np.tile(np.arange(f * f), (w * h, 1)), axis=1)
    cells = np.take_along_axis(cells, perm, axis=1)
    g = cells.reshape(h, w, f, f).transpose(0, 2, 1, 3).reshape(h * f, w * f).astype(np.uint8)
    assert set(np.unique(block_sums(g, f))) == set(range(n))
    return g
