"""The grids, sizes and planted frames the CLAHE tests share (tests/test_clahe_model.py asserts their premises on the model,
tests/test_clahe_tables.py and tests/test_clahe_frame.py run them on the GPU) -- TEST INFRASTRUCTURE ONLY."""
import numpy as np

from helpers import clahe_np as cnp
from helpers import tone_np as tnp

# name -> (W, H, tiles_x, tiles_y) of the context
GRIDS = {"1x1": (64, 48, 1, 1), "8x8": (64, 48, 8, 8), "3x2": (64, 48, 3, 2), "8x8-uneven": (70, 50, 8, 8), "tx==W": (8, 48, 8, 8)}
# reduced frames: the context, and the factors its full-size source comes in
REDUCED = (32, 24, 8, 8)
FACTORS = (1, 2, 3, 4)
# every (axis size, tiles) pair the GPU tests convert, and the pairs the rule was first checked on
AXES = ({(w, tx) for w, h, tx, ty in GRIDS.values()} | {(h, ty) for w, h, tx, ty in GRIDS.values()} |
        {(f * REDUCED[0], REDUCED[2]) for f in FACTORS} | {(f * REDUCED[1], REDUCED[3]) for f in FACTORS} |
        {(f * REDUCED[0], 3) for f in FACTORS} | {(f * REDUCED[1], 2) for f in FACTORS} |
        {(64, 8), (70, 8), (70, 3), (8, 8), (9, 8), (64, 1)} |
        # the single cases: a tile of several chunks, the very wide frames, the 6 x 4 context, the levels' and streams' settings
        {(256, 2), (130, 1), (256, 1), ((1 << 19) - 4, 8), (1 << 19, 8), (6, 6), (4, 4), (64, 2), (48, 3), (128, 8), (96, 8), (128, 3),
         (96, 2), (70, 3), (50, 2)})

# Frames whose tile (0, 0) holds `distinct` different values, one of them on every pixel to spare: with plateau 1 the excess is
# n_t - distinct, and the heavy value's count is n_t - distinct + 1.  expect: what the model must say of that tile.
#   3x2 at 64 x 48: tile (0, 0) is 21 x 24 = 504 pixels;  8x8: 8 x 6 = 48;  1x1: 3072
PLANTED = {
    "r==0": dict(grid="3x2", bits=8, distinct=248, plateau=1, expect=dict(n=504, E=256, q=1, r=0)),
    "r==1": dict(grid="3x2", bits=8, distinct=247, plateau=1, expect=dict(E=257, q=1, r=1, step=256)),
    "r==L-1": dict(grid="3x2", bits=8, distinct=249, plateau=1, expect=dict(E=255, q=0, r=255, step=1)),
    "r>L/2": dict(grid="3x2", bits=8, distinct=48, plateau=1, expect=dict(E=456, q=1, r=200, step=1)),
    "step==5": dict(grid="3x2", bits=8, distinct=198, plateau=1, expect=dict(E=306, q=1, r=50, step=5)),
    "flat-tile": dict(grid="3x2", bits=8, distinct=1, plateau=1, expect=dict(n=504, E=503, top=504, q=1, r=247, step=1)),
    "flat-frame-10bit": dict(grid="1x1", bits=10, distinct=1, plateau=1, expect=dict(n=3072, E=3071, q=2, r=1023, L=1024, step=1)),
    "hit": dict(grid="3x2", bits=8, distinct=200, plateau=305, expect=dict(top=305, E=0)),
    "hit-1": dict(grid="3x2", bits=8, distinct=200, plateau=304, expect=dict(top=305, E=1, q=0, r=1, step=256)),
    "hit+1": dict(grid="3x2", bits=8, distinct=200, plateau=306, expect=dict(top=305, E=0)),
    "hit-16bit": dict(grid="8x8", bits=16, distinct=10, plateau=39, expect=dict(n=48, top=39, E=0)),
    "hit-1-16bit": dict(grid="8x8", bits=16, distinct=10, plateau=38, expect=dict(top=39, E=1, q=0, r=1, step=65536)),
    "hit+1-16bit": dict(grid="8x8", bits=16, distinct=10, plateau=40, expect=dict(top=39, E=0)),
    "flat-tile-16bit": dict(grid="8x8", bits=16, distinct=1, plateau=1, expect=dict(E=47, q=0, r=47, step=1394)),
}


def planted(name):
    """(frame [H,W] uint16, tone map) of a PLANTED case."""
    case = PLANTED[name]
    w, h, tx, ty = GRIDS[case["grid"]]
    base = tnp.uniform(w, h, seed=len(name)) >> (16 - case["bits"])
    px, _ = cnp.plant_distinct(base, case["bits"], tx, ty, 0, 0, case["distinct"], seed=case["distinct"])
    return px, cnp.clahe(tx, ty, case["plateau"], case["bits"])


def content(name, w, h, bits, seed=0):
    """The frames of the table tests by name."""
    if name == "uniform":    # spread over the 16 bits, no value twice: every bin <= 1
        return np.random.default_rng(seed).choice(65536, size=w * h, replace=False).astype(np.uint16).reshape(h, w)
    if name == "flat":
        return tnp.flat(w, h, min(7123, (1 << bits) - 1))
    if name == "two_valued":
        return tnp.two_valued(w, h, 100, min(40000, (1 << bits) - 2), seed)
    if name == "thermal":
        return tnp.thermal(w, h, seed)
    if name == "over_depth":
        return tnp.over_depth(w, h, seed)
    if name == "halves":
        return cnp.halves(w, h, seed=seed)
    raise ValueError(name)
