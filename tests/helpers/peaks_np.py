"""The ranked-peaks rule of include/nmi_hip.h ("Ranked peaks") as a direct greedy loop in numpy, and the tables the tests rank
-- TEST INFRASTRUCTURE ONLY.

find_peaks(table, num, K, radius) -> (keys uint64 [K], count): uint64 keys, axis coordinates from np.unravel_index, one argmax
and one box test per round.  It shares nothing with the kernel (csrc/nmi_peaks.hip: lanes, register masks, an LDS bitmap) nor
with the host twin (host/nmi_peaks_host.cpp: an odometer over the box) but the rule.
Peak j does not depend on K (selection only STOPS after K peaks), so ranked(...) computes the model once for the largest K and
the tests take prefixes of it.
Every builder is deterministic (seeded from the case), so the CPU and the GPU tier see the same bytes.
"""
import functools
import itertools
import zlib

import numpy as np

MAX_K = 64
U32 = np.uint64(0xFFFFFFFF)


def keys_of(table):
    """nmi_key_pack of every cell, as uint64: score bits (-0.0 as 0.0) above, 0xFFFFFFFF - index below; 0 = does not qualify."""
    t = np.ascontiguousarray(table, np.float32).reshape(-1)
    with np.errstate(invalid="ignore"):
        qualifies = t >= 0                      # NaN and negatives: False; -0.0: True
        bits = np.where(t == 0, np.uint32(0), t.view(np.uint32)).astype(np.uint64)
    keys = (bits << np.uint64(32)) | (U32 - np.arange(t.size, dtype=np.uint64))
    return np.where(qualifies, keys, np.uint64(0))


def coordinates(num):
    """int64 [6][cells]: row a = the coordinate on axis a of every cell (axis 0 fastest, nmi_sk_linear_index's order)."""
    n = int(np.prod(num, dtype=np.int64))
    return np.stack(np.unravel_index(np.arange(n), tuple(int(v) for v in reversed(num))))[::-1].astype(np.int64)


def find_peaks(table, num, K, radius):
    keys = keys_of(table)
    assert keys.size == int(np.prod(num, dtype=np.int64)) and 1 <= K <= MAX_K
    at = coordinates(num)
    r = np.asarray(radius, np.int64)[:, None]
    live = keys != 0
    out = []
    while len(out) < K and live.any():
        i = int(np.where(live, keys, np.uint64(0)).argmax())    # (non-zero keys are distinct: the index is in them)
        out.append(keys[i])
        live &= ~(np.abs(at - at[:, i:i + 1]) <= r).all(axis=0)
    return np.array(out + [0] * (K - len(out)), np.uint64), len(out)


def prefix(model, K):
    """The answer for K <= the K the model was computed for."""
    keys, count = model
    return keys[:K].copy(), min(count, K)


# ---- the case list ---------------------------------------------------------------------------------------------------------------
SHAPES = [(1, 1, 1, 1, 1, 1), (3, 1, 1, 1, 1, 1), (3, 3, 3, 3, 3, 3), (3, 3, 3, 3, 3, 1), (1, 3, 3, 3, 3, 3),
          (5, 13, 1, 1, 1, 1),                                                  # 65 cells: one past a wavefront
          (1023, 1, 1, 1, 1, 1), (32, 32, 1, 1, 1, 1), (41, 25, 1, 1, 1, 1),      # 1023, 1024, 1025: around one cell per lane
          (8, 8, 8, 4, 4, 4),                                                   # 32,768
          (16, 16, 16, 4, 2, 2)]                                                # 65,536: the largest
TOO_LARGE = (65537, 1, 1, 1, 1, 1)
RADII = [(0,) * 6, (1,) * 6, (1, 0, 2, 0, 1, 3), (100,) * 6]
KS = (1, 2, 63, 64)
CONTENTS = ("random", "equal", "negative", "nan", "few", "zeros", "inf", "holes", "corners", "seam")


def shape_id(num):
    return "x".join(str(v) for v in num)


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def linear(num, idx6):
    lin = 0
    for a in reversed(range(6)):
        lin = lin * num[a] + idx6[a]
    return lin


def corner_cells(num):
    """The cells whose every coordinate is 0 or num - 1."""
    return sorted({linear(num, c) for c in itertools.product(*[(0, n - 1) for n in num])})


def seam_cells(num):
    """Both sides of the axis 2 / axis 3 boundary -- where the render index ends and the warp index begins -- of the first, a
    middle and the last warp step: the last render of a warp and the first render of the next."""
    S = num[0] * num[1] * num[2]
    n = S * num[3] * num[4] * num[5]
    cells = {S - 1}
    for w in sorted({1, (n // S) // 2, n // S - 1}):
        if 1 <= w < n // S:
            cells |= {w * S - 1, w * S}
    return sorted(cells)


def table(num, content):
    """float32 [cells] of the case."""
    n = int(np.prod(num, dtype=np.int64))
    rng = _rng("peaks", tuple(num), content)
    if content == "random":
        t = rng.uniform(0, 2, n)
    elif content == "equal":
        t = np.full(n, 0.5)
    elif content == "negative":
        t = -rng.uniform(0.1, 2, n)
    elif content == "nan":
        t = np.full(n, np.nan)
    elif content == "few":          # fewer qualifying cells than the larger K
        t = -rng.uniform(0.1, 2, n)
        pick = rng.choice(n, min(n, 3), replace=False)
        t[pick] = rng.uniform(0, 2, pick.size)
    elif content == "zeros":        # zeros and -0.0 only: every cell qualifies with the same score
        t = np.where(rng.random(n) < 0.5, 0.0, -0.0)
    elif content == "inf":
        t = rng.uniform(0, 2, n)
        t[int(rng.integers(0, n))] = np.inf
    elif content == "holes":
        t = rng.uniform(0, 2, n)
        u = rng.random(n)
        t[u < 0.1] = np.nan
        t[(u >= 0.1) & (u < 0.2)] = -t[(u >= 0.1) & (u < 0.2)] - 0.1
    elif content == "corners":      # equal maxima on every corner of the grid, over a low random floor
        t = rng.uniform(0, 1, n)
        t[corner_cells(num)] = 1.5
    elif content == "seam":         # equal maxima either side of the render / warp boundary
        t = rng.uniform(0, 1, n)
        t[seam_cells(num)] = 1.75
    else:
        raise KeyError(content)
    return t.astype(np.float32)


@functools.lru_cache(maxsize=None)
def ranked(num, content, radius):
    """The model's answer for K = MAX_K (callers take prefix(); they do not write into it)."""
    return find_peaks(table(num, content), num, MAX_K, radius)


def cases(num):
    """[(content, radius, K)] of a shape: everything with everything."""
    return [(c, r, k) for c in CONTENTS for r in RADII for k in KS]
