"""The cases the valid-range pipeline tests share (tests/test_valid_pipeline_plan.py, test_valid_level.py, test_valid_stream.py):
sizes, the planted deep frames, their range and tone maps, and the premises those frames must meet -- TEST INFRASTRUCTURE ONLY.

A pipeline frame is an 8-bit frame lifted to 14 bits (tests/test_tone_pipeline.py's `deep`: 9000 + 3 g + noise) at f times the
search size, with planted "no measurement" values: 0 in a few blobs and in scattered single source pixels, 65535 in a handful of
dead pixels.  The range is (1, 16383): both sentinels are outside it, every lifted value inside."""
import numpy as np

from helpers import clahe_np as cnp
from helpers import tone_np as tnp
from helpers import valid_np as vnp

BITS = 14
RANGE = (1, 16383)
# 64 x 48: whole quads, rows of 16-byte chunks; 52 x 38: frame rows not 16-byte aligned (the warp kernel on the forked branch);
# 54 x 38: W % 4 != 0, the conversion's scalar output path writes the grey / mask pair
SIZES = [(64, 48), (52, 38), (54, 38)]
FACTORS = (1, 2)
SCATTER = 0.03      # share of the SOURCE pixels that are lone holes
DEAD = 6            # dead pixels at 65535


def tone_maps():
    """label -> tone_np / clahe_np dict: the four the pipeline tests run."""
    return {"shift": tnp.tone(tnp.SHIFT, BITS), "pct": tnp.tone(tnp.PERCENTILE, BITS, p_lo=100, p_hi=100),
            "equalize": tnp.tone(tnp.EQUALIZE, BITS), "clahe3x2": cnp.clahe(3, 2, 0, BITS)}


def capi_tone(capi, tm):
    return cnp.capi_tone(capi, tm) if vnp.tiled(tm) else tnp.capi_tone(capi, tm)


def lift(gray, seed=0):
    """[Hs,Ws] uint8 -> uint16, 14 bits in use: test_tone_pipeline.deep's bright band."""
    g = np.asarray(gray, np.int64)
    return (9000 + 3 * g + np.random.default_rng(seed).integers(0, 3, g.shape)).astype(np.uint16)


def spread(gray, f, seed=0):
    """[H,W] uint8 -> [f H, f W] uint8 (test_reduce_level.full_size's rule): each pixel over its block, a fine texture on top."""
    if f == 1:
        return np.asarray(gray, np.uint8)
    big = np.kron(np.asarray(gray, np.int64), np.ones((f, f), np.int64))
    return np.clip(big + np.random.default_rng(seed).integers(-9, 10, big.shape), 0, 255).astype(np.uint8)


def plant(px, f, seed=0, sentinel=65535):
    """Holes into a copy of the [f H, f W] pixels: three blobs of 0 (one reaching into the hood's rows at the bottom, none covering
    them), lone 0 pixels at SCATTER of the source pixels, DEAD pixels at `sentinel`."""
    px = np.array(px, np.uint16, copy=True)
    hs, ws = px.shape
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:hs, 0:ws]
    # (centre x, centre y, radius x, radius y) as shares of the frame
    for cx, cy, rx, ry in ((0.30, 0.35, 0.16, 0.18), (0.72, 0.55, 0.13, 0.20), (0.45, 0.93, 0.10, 0.09)):
        px[((xx - cx * ws) / (rx * ws)) ** 2 + ((yy - cy * hs) / (ry * hs)) ** 2 <= 1.0] = 0
    px[rng.random((hs, ws)) < SCATTER] = 0
    px.reshape(-1)[rng.choice(ws * hs, size=DEAD, replace=False)] = sentinel
    return px


def frame(gray, f, seed=0):
    """The pipeline frame of an 8-bit [H,W] frame at factor f: [f H, f W] uint16."""
    return plant(lift(spread(gray, f, seed), seed), f, seed)


def hood(w, h):
    """test_masked_level.hood_mask: the bottom sixth and a mount in the top-left corner unusable."""
    m = np.ones((h, w), np.uint8)
    m[h - h // 6:] = 0
    m[:h // 8, :w // 10] = 0
    return m


def premises(px, f, rng=RANGE, bits=BITS):
    """What a planted frame must be for the pipeline tests to mean anything; asserted on the CPU for the stand-in frames and again,
    cheaply, on every frame a GPU test makes.  Conditions on the inputs, never on the code under test."""
    hs, ws = px.shape
    h, w = hs // f, ws // f
    for tm in (tnp.tone(tnp.EQUALIZE, bits), tnp.tone(tnp.PERCENTILE, bits, p_lo=100, p_hi=100)):
        assert (vnp.table(px, tm, rng)[0] != vnp.table(px, tm, vnp.OFF)[0]).any(), tm["mode"]
    m = vnp.mask(px, f, rng)
    assert set(np.unique(m)) == {0, 1}
    zero = 1.0 - float(m.mean())
    assert 0.10 <= zero <= 0.50, zero                       # the masked search neither ignores it nor runs out of pixels
    hd = hood(w, h)
    both = vnp.mask(px, f, rng, hd)
    assert (both != hd).any() and (both != m).any()
    if f == 2:                                              # an output pixel lost to exactly one of its four source pixels
        bad = (~vnp.valid(px, rng)).astype(np.int64)
        per_block = bad.reshape(h, f, w, f).sum(axis=(1, 3))
        assert (per_block == 1).any()
    return zero
