"""Stacks with exactly controlled level sets for the few-levels path (csrc/nmi_fewlevels_kernel.hip) -- TEST INFRASTRUCTURE ONLY.

exact_levels(shape, levels, rng) -> uint8 stack whose set of distinct values is exactly `levels`.
plant(stack, image, pos, value)  -> copy of `stack` with ONE pixel of a value that occurs nowhere else in it.
The case tables below are module-level constants: the CPU tests of tests/test_few_levels_edges.py check every stack they describe
(exact sets, sensitivity of every planted pixel, coverage of the seen[] words) and its GPU tests run the same stacks.  Every
builder is deterministic (seeded from the case), so both tiers see the same bytes.
"""
import functools
import zlib

import numpy as np

W, H = 64, 48                       # the frame of every case that does not name another
BOUNDARY = (0, 31, 32, 63, 64, 127, 128, 255)   # first / last bits of the probe's 32-bit presence words
PROBE_SLICES = 4                    # launch_levels: workgroups per image
PROBE_BLOCK, PROBE_LOADS = 1024, 4  # nmi_levels_kernel: lanes, loads in flight per lane


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def exact_levels(shape, levels, rng):
    """Random fill from `levels`, then every level once at a position of its own."""
    lv = np.unique(np.asarray(levels, np.int64))
    assert lv.size >= 1 and lv[0] >= 0 and lv[-1] <= 255 and lv.size <= int(np.prod(shape))
    lv = lv.astype(np.uint8)
    stack = lv[rng.integers(0, lv.size, int(np.prod(shape)))]
    stack[rng.choice(stack.size, lv.size, replace=False)] = lv
    return stack.reshape(shape)


def exact_levels_per_image(shape, sets, rng):
    """Image i holds exactly sets[i]."""
    assert len(sets) == shape[0]
    return np.stack([exact_levels(shape[1:], s, rng) for s in sets])


def plant(stack, image, pos, value):
    """One pixel (flat index `pos` of image `image`) of a value the stack does not hold yet."""
    assert not (stack == value).any(), value
    out = stack.copy()
    out[image].reshape(-1)[pos] = value
    return out


def draw(n, rng, lo=0, hi=256):
    """n distinct intensities from lo .. hi - 1, sorted."""
    return tuple(int(v) for v in np.sort(rng.choice(np.arange(lo, hi), n, replace=False)))


# ---- exact joint sizes (section 2, copy-count and size edges) --------------------------------------------------------------------
# name -> (render set, warp set, few-levels expected at the default limit).  Sets drawn at random from 0..255 unless fixed.
def _joint_cases():
    cases = {}
    for nr, nw, few in [(32, 32, True), (25, 41, True), (64, 32, True), (41, 50, True), (64, 64, True), (256, 16, True), (16, 256, True),
                        (17, 241, False), (256, 1, True), (1, 256, True), (1, 1, True)]:
        rng = _rng("joint", nr, nw)
        cases[f"{nr}x{nw}"] = (draw(nr, rng), draw(nw, rng), few)
    cases["boundary8x8"] = (BOUNDARY, BOUNDARY, True)
    cases["boundary8x4"] = (BOUNDARY, (15, 16, 143, 144), True)
    return cases


JOINT_CASES = _joint_cases()
ALL_ZERO_JOINTS = ("256x1", "1x256", "1x1")   # one stack constant: every score is 0 by the all-zero guard (NMI.cu:342-362)
# (case, NMI_OPT_FEWLEVELS_BINS, taken): a joint of exactly L is taken, L + 1 is not
LIMIT_CASES = [("25x41", 1025, True), ("25x41", 1024, False), ("32x32", 1024, True), ("32x32", 1023, False)]


def joint_stacks(name, S=9, Wn=9):
    rs_set, ws_set, _ = JOINT_CASES[name]
    rng = _rng("joint-stack", name, S, Wn)
    return exact_levels((S, H, W), rs_set, rng), exact_levels((Wn, H, W), ws_set, rng)


# ---- levels absent from an image ---------------------------------------------------------------------------------------------------
ABSENT_SETS = (draw(12, _rng("absent", 0)), draw(10, _rng("absent", 1)))


def absent_stacks(S=9, Wn=9):
    """Image i uses the even-ranked half of its stack's set when i is even, the odd-ranked half otherwise."""
    rng = _rng("absent-stack")
    r, w = ABSENT_SETS
    return (exact_levels_per_image((S, H, W), [r[i % 2::2] for i in range(S)], rng),
            exact_levels_per_image((Wn, H, W), [w[i % 2::2] for i in range(Wn)], rng))


# ---- background rule off, 256 bins -------------------------------------------------------------------------------------------------
# name -> (render set, warp set); "late0": 0 is in both stacks but in neither's image 0
_WITH0, _NO0_R, _NO0_W = (0, 40, 90, 200), (7, 40, 90, 200), (3, 60, 120, 180, 250)
ZERO_CASES = {"both": (_WITH0, (0, 60, 120, 180, 250)), "render_only": (_WITH0, _NO0_W), "warp_only": (_NO0_R, (0, 60, 120, 180, 250)),
              "neither": (_NO0_R, _NO0_W), "late0": (_WITH0, (0, 60, 120, 180, 250))}


def zero_stacks(name, S=9, Wn=9):
    r, w = ZERO_CASES[name]
    rng = _rng("zero-stack", name)
    if name != "late0":
        return exact_levels((S, H, W), r, rng), exact_levels((Wn, H, W), w, rng)
    return (exact_levels_per_image((S, H, W), [r[1:]] + [r] * (S - 1), rng),
            exact_levels_per_image((Wn, H, W), [w[1:]] + [w] * (Wn - 1), rng))


# ---- reduced bins with the rule on -------------------------------------------------------------------------------------------------
# (bins, number of render bins, number of warp bins): the raw values differ inside every bin
BIN_CASES = [(64, 10, 7), (64, 64, 64), (16, 9, 16), (16, 16, 5)]


def bin_sets(bins, nrb, nwb):
    """-> (render bins, warp bins, raw render values, raw warp values): at least two raw values in every bin."""
    shift = {64: 2, 16: 4}[bins]
    rng = _rng("bins", bins, nrb, nwb)
    out = []
    for n in (nrb, nwb):
        b = draw(n, rng, 0, bins)
        raw = []
        for v in b:
            raw += [(v << shift) + int(o) for o in rng.choice(1 << shift, 2 + int(rng.integers(0, (1 << shift) - 1)), replace=False)]
        out.append((b, tuple(sorted(raw))))
    return out[0][0], out[1][0], out[0][1], out[1][1]


def bin_stacks(bins, nrb, nwb, S=9, Wn=9):
    _, _, rr, wr = bin_sets(bins, nrb, nwb)
    rng = _rng("bin-stack", bins, nrb, nwb)
    return exact_levels((S, H, W), rr, rng), exact_levels((Wn, H, W), wr, rng)


# ---- one planted pixel -------------------------------------------------------------------------------------------------------------
PLANT_FRAMES = [(32, 1), (48, 3), (64, 48), (64, 4097)]
PLANT_SETS = ((10, 60, 110, 160, 210), (25, 75, 125, 225))   # render / warp stacks before the plant
PLANT_VALUE = (135, 150)                                        # planted in a render / in a warp: between two ranks of its stack


def probe_slice_chunks(npix):
    """Chunks per slice of nmi_levels_kernel (16-byte chunks, ceil(nchunks / slices))."""
    nchunks = npix // 16
    return nchunks, (nchunks + PROBE_SLICES - 1) // PROBE_SLICES


def plant_positions(w, h):
    """Byte offsets in an image's memory: first byte, 15, 16, last byte, first byte of the last chunk, the last byte before and the
    first byte after every slice boundary of the probe."""
    npix = w * h
    nchunks, per = probe_slice_chunks(npix)
    pos = {0, 15, 16, npix - 1, (nchunks - 1) * 16}
    for k in range(1, PROBE_SLICES):
        if k * per < nchunks:
            pos |= {k * per * 16 - 1, k * per * 16}
    return sorted(pos)


def flipped(pos, w, h):
    """The byte that frame position `pos` meets in a bottom-up render (NMI.cu:82: frame row y meets render row H-1-y)."""
    y, x = divmod(pos, w)
    return (h - 1 - y) * w + x


def plant_cases(w, h, bottom_up, which):
    """[(image, byte offset in that image's memory)] for a plant in a render (which = 0) or a warp (1) of a 2 x 2 search.  A
    bottom-up render takes every position twice: as it lies in memory (what the probe's slices see) and where the flip moves it
    (placed by the frame row it meets: what the rank images and the scoring kernel see).  The plants alternate between the two
    images; the last byte and the last chunk are always in the LAST image of the stack as well."""
    pos = plant_positions(w, h)
    if which == 0 and bottom_up:
        pos = sorted(set(pos) | {flipped(p, w, h) for p in pos})
    npix = w * h
    cases = [(i % 2, p) for i, p in enumerate(pos)]
    cases += [(1, p) for p in (npix - 1, (npix // 16 - 1) * 16) if (1, p) not in cases]
    return cases


@functools.lru_cache(maxsize=None)
def plant_base(w, h):
    """(callers do not write into these: plant() copies)"""
    rng = _rng("plant-base", w, h)
    return exact_levels((2, h, w), PLANT_SETS[0], rng), exact_levels((2, h, w), PLANT_SETS[1], rng)


def planted(w, h, which, image, pos):
    """-> (render stack, warp stack) of the case."""
    rs, ws = plant_base(w, h)
    if which == 0:
        return plant(rs, image, pos, PLANT_VALUE[0]), ws
    return rs, plant(ws, image, pos, PLANT_VALUE[1])


def nearest_level(levels, value):
    return min(levels, key=lambda v: (abs(int(v) - int(value)), v))


# ---- hot bin -------------------------------------------------------------------------------------------------------------------------
def hot_stacks(w=640, h=480):
    """Constant stacks except one planted pixel each: candidate (render 0, warp 0) has 307,199 hits in one bin."""
    rs = plant(np.full((2, h, w), 77, np.uint8), 0, w * h - 1, 130)
    ws = plant(np.full((2, h, w), 201, np.uint8), 1, 16 * 1024 + 5, 9)
    return rs, ws


# ---- 27 x 27: candidates per workgroup, visiting order, shards -----------------------------------------------------------------------
GRID27_SETS = ((4, 50, 99, 150, 201, 252), (0, 64, 128, 192, 255))
GRID27_FIRST = 3                       # renders 0 .. 2 hold only the first four levels (a shard with fewer levels than the stack)
RENDER_SHARDS = [(0, 3), (3, 9), (9, 18), (18, 27)]
WARP_SHARDS = [(0, 9), (9, 18), (18, 27)]


def grid27_stacks():
    rng = _rng("grid27")
    r, w = GRID27_SETS
    return (exact_levels_per_image((27, H, W), [r[:4]] * GRID27_FIRST + [r] * (27 - GRID27_FIRST), rng), exact_levels((27, H, W), w, rng))


# ---- one context, changing sets ----------------------------------------------------------------------------------------------------
def changing_sets():
    """A: 40 x 50 levels; B: 3 x 2 levels none of which A holds."""
    rng = _rng("changing")
    pool = rng.permutation(256)
    a = (tuple(sorted(int(v) for v in pool[:40])), tuple(sorted(int(v) for v in pool[40:90])))
    b = (tuple(sorted(int(v) for v in pool[90:93])), tuple(sorted(int(v) for v in pool[93:95])))
    return a, b


def changing_stacks():
    a, b = changing_sets()
    rng = _rng("changing-stack")
    return ((exact_levels((9, H, W), a[0], rng), exact_levels((9, H, W), a[1], rng)),
            (exact_levels((9, H, W), b[0], rng), exact_levels((9, H, W), b[1], rng)))


# ---- the general kernel as probe (section 3) -----------------------------------------------------------------------------------------
def seen_slot(bin_):
    """LevelPlan::seen: bin -> (word within the stack's 16 words, bit): bit k of word i is bin i + 16 k below 128 and
    i + 16 (k - 8) + 128 above."""
    i, k = bin_ % 16, (bin_ % 128) // 16 + (8 if bin_ >= 128 else 0)
    return i, k


def _partitions():
    """Eight random pairs of sets that between them hold every intensity 0..255 on each side (32 x 32 each)."""
    rng = _rng("partition")
    pr, pw = rng.permutation(256), rng.permutation(256)
    return [(tuple(sorted(int(v) for v in pr[32 * i:32 * i + 32])), tuple(sorted(int(v) for v in pw[32 * i:32 * i + 32]))) for i in range(8)]


PARTITION_SETS = _partitions()
# name -> (bins, render set, warp set); sets are raw intensities, counts are in bins
PROBE_CASES = {"boundary": (256, BOUNDARY, (15, 16, 143, 144)),
               "256x16": (256,) + JOINT_CASES["256x16"][:2],
               "16x256": (256,) + JOINT_CASES["16x256"][:2]}
PROBE_CASES.update({f"partition{i}": (256, r, w) for i, (r, w) in enumerate(PARTITION_SETS)})
PROBE_CASES["bins64"] = (64,) + bin_sets(64, 10, 7)[2:]


def probe_counts(name):
    bins, r, w = PROBE_CASES[name]
    shift = {256: 0, 64: 2}[bins]
    return len({v >> shift for v in r}), len({v >> shift for v in w})


def probe_stacks(name, S=3, Wn=3):
    _, r, w = PROBE_CASES[name]
    rng = _rng("probe-stack", name)
    return exact_levels((S, H, W), r, rng), exact_levels((Wn, H, W), w, rng)


# default workgroups: a factor of two or more inside / outside the 4096 limit
def verdict_stacks(S=12, Wn=12):
    rng = _rng("verdict")
    few = (exact_levels((S, H, W), draw(40, rng), rng), exact_levels((Wn, H, W), draw(50, rng), rng))       # 2000 <= 2048
    many = (exact_levels((S, H, W), draw(100, rng), rng), exact_levels((Wn, H, W), draw(90, rng), rng))     # 9000 >= 8192
    return few, many
