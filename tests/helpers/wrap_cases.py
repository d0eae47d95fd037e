"""Case tables for tests/test_mask_search_edges.py -- TEST INFRASTRUCTURE ONLY.

Images whose joint histogram is controlled exactly, for the masked and covered grid searches (csrc/nmi_masked_kernel.hip,
csrc/nmi_covered_kernel.hip, csrc/nmi_mask_device.h):

planted   a render / warped-frame pair in which listed raw pairs occur an exact number of times.
wraps     the premise function: does the optimistic pass (non-returning adds on two 16-bit fields per word) fail its count test?
CASES     group 1, one planted candidate on a count boundary of a field (65,535 / 65,536 / 65,537 ...), in a 2 x 2 grid with
          three textured candidates.
GRIDS     group 2, grids of nearly flat and textured images in which a known subset of the candidates wraps.
TERMS     group 3, small frames whose counts and lengths sit on the 4095 / 4096 / 4097 boundary of the per-count term table.

Every image here is in FRAME coordinates (top-down); stacks() flips renders and render masks for a bottom-up context.

score_f64 is an independent float64 score from exact integer counts (np.log2 in double, the SUC / ENMI form of
oracle/nmi_oracle_np.py).  Largest |rounded model - score_f64| over every candidate of CASES and TERMS, both searches, measured
on the CPU tier: 1.44e-6 (F64_SEEN; on a candidate of T3 with all but three of 2,473 pixels in one bin, where the score is a
quotient of sums near 1e-2); the tests assert 4 x that (another libm may round a logarithm the other way).
"""
import functools
from collections import namedtuple

import numpy as np

from helpers import covered_np as cnp
from helpers import masked_np as mnp
from oracle import binding as oc

SHIFT = {256: 0, 64: 2}
F64_SEEN = 1.44e-6
FRAMES = {"A": (512, 129), "B": (512, 258), "R": (257, 257), "Amis": (512, 129), "T": (128, 40), "T2": (96, 43), "T3": (64, 48)}
BYTE_PATH = ("R", "Amis")  # frames whose rows are not whole aligned 16-byte chunks


def planted(w, h, bins, seed, layout="scattered"):
    """-> (render [h, w], warped [h, w]) uint8, render top-down.  bins: ((d1, d2), n) raw pairs, each occurs exactly n times;
    every other pixel is random texture in 1..254 that never forms a listed pair (so a pair listed with n = 0 never occurs).
    layout "scattered": all pixels permuted; "runs": each planted pair contiguous (from pixel 37, off every 4- and 16-pixel
    boundary), so one lane's batch of four and one wavefront's chunks meet the same word again and again."""
    assert layout in ("scattered", "runs")
    rng = np.random.default_rng(seed)
    n = w * h
    total = sum(k for _, k in bins)
    assert total <= n and len({p for p, _ in bins}) == len(bins)
    r = rng.integers(1, 255, n, dtype=np.uint8)
    f = rng.integers(1, 255, n, dtype=np.uint8)
    listed = np.zeros((256, 256), bool)
    for (d1, d2), _ in bins:
        listed[d1, d2] = True
    for _ in range(256):
        hit = listed[r, f]
        if not hit.any():
            break
        f[hit] = f[hit] % 254 + 1  # another value of 1..254
    assert not listed[r, f].any()
    pos = min(37, n - total)
    for (d1, d2), k in bins:
        r[pos:pos + k], f[pos:pos + k] = d1, d2
        pos += k
    if layout == "scattered":
        p = rng.permutation(n)
        r, f = r[p], f[p]
    return r.reshape(h, w), f.reshape(h, w)


def wraps(joint_all):
    """Does the optimistic pass fail for this candidate?  joint_all [256, 256]: the histogram of every pixel the mask lets
    through -- before the background rule where the kernel counts all (rule on; rule off at 256 bins), after the shift.  A word
    holds the bins (d1, d2) and (d1, d2 + 128) as 16-bit fields, the low one carrying into the high one."""
    j = np.asarray(joint_all, np.int64)
    lo, hi = j[:, :128], j[:, 128:]
    return bool((lo >= 65536).any() or (hi + lo // 65536 >= 65536).any())


def texture(shape, seed):
    return np.random.default_rng(seed).integers(1, 255, shape, dtype=np.uint8)


def holes(shape, allowed, n, rng, values=(1,)):
    """A mask of `values` (nonzero bytes, drawn at random) with n zeros among the positions `allowed` (bool, same shape)."""
    m = rng.choice(np.asarray(values, np.uint8), size=shape)
    idx = np.flatnonzero(allowed)
    m.reshape(-1)[rng.choice(idx, n, replace=False)] = 0
    return m


def stacks(case):
    """-> (rs, ws, wm, rm) as the searches take them: renders and render masks flipped for a bottom-up context."""
    flip = (lambda a: a[:, ::-1]) if case["cfg"].get("bottom_up", True) else (lambda a: a)
    return (np.ascontiguousarray(flip(case["rs"])), case["ws"], case["wm"], np.ascontiguousarray(flip(case["rm"])))


def models(case):
    """-> (masked model, covered model): masked_np.masked_search and covered_np.covered_search under oracle.binding.rounded()."""
    rs, ws, wm, rm = stacks(case)
    c = case["cfg"]
    a = (SHIFT[c.get("bins", 256)], c.get("use_bg", True), c.get("bottom_up", True), c.get("mode", oc.MODE_SUC))
    return mnp.masked_search(rs, ws, wm, *a), cnp.covered_search(rs, ws, wm, rm, *a)


def pair_masks(case, covered):
    """-> bool [Wn, S, H, W] in frame coordinates: the pixels a candidate's masks let through."""
    wm, rm = case["wm"] != 0, case["rm"] != 0
    return wm[:, None] & rm[None] if covered else np.broadcast_to(wm[:, None], (len(wm), len(rm)) + wm.shape[1:])


def hist(case, w, s, covered, count_all=False):
    """-> (joint, h1, h2, len) of candidate (w, s) by the model's rule; count_all: before the background rule."""
    c = case["cfg"]
    m = pair_masks(case, covered)[w, s]
    j, h1, h2 = mnp.masked_hist(case["rs"][s], case["ws"][w], m, SHIFT[c.get("bins", 256)], count_all or c.get("use_bg", True), False)
    return j, h1, h2, int(m.sum())


def optimistic(cfg):
    """Is there an optimistic launch at all?  (Rule off below 256 bins is exact from the start.)"""
    return cfg.get("use_bg", True) or cfg.get("bins", 256) == 256


def score_f64(render, warped, mask, shift, use_bg, mode):
    """Independent float64 score of one candidate, all images in frame coordinates: a pixel counts iff mask and (rule on or both
    raw values nonzero); len = popcount(mask), not reduced by the rule; bins = raw >> shift; p = c / len;
    a = sum p log2 p; SUC = 2 (1 - a3 / (a1 + a2)), ENMI = (a1 + a2) / a3; 0 when all three sums are 0 (or len is 0)."""
    take = mask.reshape(-1) != 0
    length = int(take.sum())
    r, f = render.reshape(-1).astype(np.int64), warped.reshape(-1).astype(np.int64)
    if not use_bg:
        take = take & (r > 0) & (f > 0)
    if length == 0 or not take.any():
        return 0.0
    r, f = r[take] >> shift, f[take] >> shift

    def plogp(codes):
        p = np.unique(codes, return_counts=True)[1].astype(np.float64) / float(length)
        return float(np.sum(p * np.log2(p)))
    a1, a2, a3 = plogp(r), plogp(f), plogp(r * 1000 + f)
    if a1 == 0.0 and a2 == 0.0 and a3 == 0.0:
        return 0.0
    return 2.0 * (1.0 - a3 / (a1 + a2)) if mode == oc.MODE_SUC else (a1 + a2) / a3


def f64_table(case, covered):
    c = case["cfg"]
    pm = pair_masks(case, covered)
    out = np.zeros(pm.shape[:2])
    for w in range(pm.shape[0]):
        for s in range(pm.shape[1]):
            out[w, s] = score_f64(case["rs"][s], case["ws"][w], pm[w, s], SHIFT[c.get("bins", 256)], c.get("use_bg", True),
                                  c.get("mode", oc.MODE_SUC))
    return out


# ======================================================================================================================================
# group 1: one planted candidate on a field boundary
# ======================================================================================================================================
# pairs: ((d1, d2), counted n); mask: holes / bytes / down (5 more occurrences, under mask zeros) / up (100 more, under zeros)
Spec = namedtuple("Spec", "frame pairs layout mask cfg wraps")
LO, HI = (9, 5), (9, 133)  # one word: fields d2 = 5 and d2 = 5 + 128


def _group1():
    t = {}

    def add(name, frame, pairs, mask="holes", cfg=None, wraps_=True, layouts=("scattered", "runs")):
        for lay in layouts:
            t[f"{name}-{lay}"] = Spec(frame, tuple(pairs), lay, mask, dict(cfg or {}), wraps_)
    for fld, pair in (("lo", LO), ("hi", HI)):
        for n in (65535, 65536, 65537):
            add(f"A-{fld}-{n}", "A", [(pair, n)], wraps_=n > 65535)
        add(f"B-{fld}-131072", "B", [(pair, 131072)])
        for frame in BYTE_PATH:
            add(f"{frame}-{fld}-65536", frame, [(pair, 65536)])
        add(f"A-{fld}-65536-bytes", "A", [(pair, 65536)], mask="bytes", layouts=("scattered",))
        add(f"A-{fld}-down", "A", [(pair, 65535)], mask="down", wraps_=False)
        add(f"A-{fld}-up", "A", [(pair, 65536)], mask="up")
        add(f"A-{fld}-65536-topdown", "A", [(pair, 65536)], cfg=dict(bottom_up=False))
    # 64 bins: four raw pairs of one shifted bin, 16,384 each (shifted d2 < 64: there is no high field)
    four = [((36 + k, 4 + (k * 3) % 4), 16384) for k in range(4)]
    add("A-64bins", "A", four, cfg=dict(bins=64))
    add("A-64bins-bgoff", "A", four, cfg=dict(bins=64, use_bg=False))
    add("B-lo-131071", "B", [(LO, 131071)])
    add("B-two-65536-65535", "B", [(LO, 65536), (HI, 65535)])  # the word ends as 0, with two events
    add("B-two-65535-65536", "B", [(LO, 65535), (HI, 65536)])
    add("B-two-65536-65536", "B", [(LO, 65536), (HI, 65536)])
    # rule off at 256 bins: the wrap is in row 0 / column 0, counted, detected and then cleared
    add("A-row0-lo-bgoff", "A", [((0, 5), 65536)], cfg=dict(use_bg=False))
    add("A-row0-hi-bgoff", "A", [((0, 133), 65536)], cfg=dict(use_bg=False))
    add("A-col0-bgoff", "A", [((9, 0), 65536)], cfg=dict(use_bg=False))
    # rule off at 64 bins (exact from the start): raw 0 shares bin 0 with 1..3 and is dropped, the other three count
    add("A-col0-64bins-bgoff", "A", [((36 + k, k), 16384) for k in range(4)], cfg=dict(bins=64, use_bg=False), wraps_=False,
        layouts=("runs",))
    return t


CASES = _group1()


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(rs [2], ws [2], wm [2], rm [2], cfg, spec): candidate (warp 0, render 0) is the planted one; render 1 and
    warp 1 are texture.  Mask zeros lie on texture pixels only (down / up: and on the stated number of planted ones), so the
    counted number of each planted pair is the one in the table for the masked and the covered search alike.
    In the "runs" layout the texture is the first 37 and the last few hundred pixels, so with the holes mask the optimistic
    launch takes the whole planted run through the unmasked add_chunk; the run meets masked_add_chunk's batches of four on the
    exact launch (unconditional at HIST 1), and the per-pixel optimistic form only in the down / up cases, whose zeros lie
    inside the run."""
    sp = CASES[name]
    w, h = FRAMES[sp.frame]
    seed = sum(ord(c) * (i + 1) for i, c in enumerate(name))
    rng = np.random.default_rng(seed + 1)
    extra = {"down": 5, "up": 100}.get(sp.mask, 0)
    bins = [(p, n + (extra if i == 0 else 0)) for i, (p, n) in enumerate(sp.pairs)]
    r, f = planted(w, h, bins, seed, sp.layout)
    is_planted = np.zeros((h, w), bool)
    for (d1, d2), _ in bins:
        is_planted |= (r == d1) & (f == d2)
    values = (1, 2, 255) if sp.mask == "bytes" else (1,)
    wm = np.stack([holes((h, w), ~is_planted, 50, rng, values), holes((h, w), np.ones((h, w), bool), 40, rng, values)])
    if extra:
        first = np.flatnonzero((r == bins[0][0][0]) & (f == bins[0][0][1]))
        wm[0].reshape(-1)[rng.choice(first, extra, replace=False)] = 0
    free = ~is_planted & (wm[0] != 0)
    rm = np.stack([holes((h, w), free, 3, rng), holes((h, w), free, 7, rng)])
    return dict(rs=np.stack([r, texture((h, w), seed + 2)]), ws=np.stack([f, texture((h, w), seed + 3)]), wm=wm, rm=rm, cfg=sp.cfg,
                spec=sp)


# ======================================================================================================================================
# group 2: grids in which a known subset of the candidates wraps (frame A)
# ======================================================================================================================================
PATCH = 300  # textured pixels at the end of a nearly flat image: its flat bin holds 66,048 - 300 minus the mask zeros


def nearly_flat(value, patch):
    w, h = FRAMES["A"]
    img = np.full(w * h, value, np.uint8)
    img[-PATCH:] = patch
    return img.reshape(h, w)


def _patch(seed):
    return texture(PATCH, seed)


def _grid(renders, warps, seed, same_rm=()):
    """renders / warps: lists of ("flat", value, patch seed) or ("tex", seed).  same_rm: renders that share one render mask."""
    w, h = FRAMES["A"]
    rng = np.random.default_rng(seed)

    def img(d):
        return nearly_flat(d[1], _patch(d[2])) if d[0] == "flat" else texture((h, w), d[1])
    rs, ws = np.stack([img(d) for d in renders]), np.stack([img(d) for d in warps])
    anywhere = np.ones((h, w), bool)
    wm = np.stack([holes((h, w), anywhere, 30 + 5 * k, rng) for k in range(len(warps))])
    rm = np.stack([holes((h, w), anywhere, 2 + 3 * k, rng) for k in range(len(renders))])
    for k in same_rm[1:]:
        rm[k] = rm[same_rm[0]]
    flat = [[renders[s][0] == "flat" and warps[v][0] == "flat" for s in range(len(renders))] for v in range(len(warps))]
    return dict(rs=rs, ws=ws, wm=wm, rm=rm, cfg={}, flat=np.array(flat))


# 4 x 4: renders [tex, flat, tex, flat], warps [tex, flat, flat, tex]: candidates 5, 7, 9, 11 (w * 4 + s) wrap
GRID_DEFS = {
    # warp 1's patch is render 3's: candidate (1, 3) = 7 scores 1.0
    "4x4-winner-wraps": dict(renders=[("tex", 1), ("flat", 200, 11), ("tex", 2), ("flat", 90, 12)],
                             warps=[("tex", 3), ("flat", 100, 12), ("flat", 30, 13), ("tex", 4)]),
    # warp 3 is render 2: candidate (3, 2) = 14 scores 1.0
    "4x4-winner-clean": dict(renders=[("tex", 1), ("flat", 200, 11), ("tex", 2), ("flat", 90, 12)],
                             warps=[("tex", 3), ("flat", 100, 14), ("flat", 30, 13), ("tex", 2)]),
    # renders 1 and 3 are one image under one render mask: candidates 9 and 11 tie at the top, both on the list
    "4x4-tie": dict(renders=[("tex", 1), ("flat", 200, 11), ("tex", 2), ("flat", 200, 11)],
                    warps=[("tex", 3), ("flat", 100, 14), ("flat", 30, 11), ("tex", 4)], same_rm=(1, 3)),
    "3x3-all-wrap": dict(renders=[("flat", 200, 11), ("flat", 90, 12), ("flat", 7, 13)],
                         warps=[("flat", 100, 14), ("flat", 30, 12), ("flat", 250, 15)]),
    "3x3-none-wraps": dict(renders=[("tex", 1), ("tex", 2), ("tex", 5)], warps=[("tex", 3), ("tex", 5), ("tex", 4)]),
    # 5 renders x 6 warps: 2 x 3 = 6 candidates wrap; the list is longer than any before it in the reuse sequence
    "5x6": dict(renders=[("tex", 1), ("flat", 200, 11), ("tex", 2), ("flat", 90, 12), ("tex", 6)],
                warps=[("tex", 3), ("flat", 100, 12), ("flat", 30, 13), ("tex", 2), ("flat", 60, 16), ("tex", 7)]),
}
GRID_WRAPS = {"4x4-winner-wraps": 4, "4x4-winner-clean": 4, "4x4-tie": 4, "3x3-all-wrap": 9, "3x3-none-wraps": 0, "5x6": 6}
REUSE_ORDER = ("4x4-winner-wraps", "3x3-none-wraps", "3x3-all-wrap", "5x6")


@functools.lru_cache(maxsize=None)
def grid(name):
    d = GRID_DEFS[name]
    return _grid(d["renders"], d["warps"], sum(map(ord, name)), d.get("same_rm", ()))


# ======================================================================================================================================
# group 3: term-table boundaries (no wraps)
# ======================================================================================================================================
def _zone_pair(frame, n, seed, layout, cfg):
    """A planted (255, 255) x n pair and the planted positions in image order.  255 lies outside the texture, so the bin is alone
    in its row and its column: the joint count is also both marginals'.  At 64 bins the texture keeps out of bin 63."""
    w, h = FRAMES[frame]
    r, f = planted(w, h, [((255, 255), n)], seed, layout)
    zone = np.flatnonzero(r.reshape(-1) == 255)
    if cfg.get("bins", 256) == 64:
        r[(r >= 252) & (r < 255)] -= 100
        f[(f >= 252) & (f < 255)] -= 100
    return r, f, zone


def _first(order, n, shape):
    m = np.zeros(shape[0] * shape[1], np.uint8)
    m[order[:n]] = 1
    return m.reshape(shape)


def _with_zone(img, zone, n, seed):
    """img (255 on the whole zone) with 255 on the first n zone positions only, texture of 1..251 on the rest of the zone."""
    out = img.copy().reshape(-1)
    out[zone[n:]] = np.minimum(texture(len(zone), seed), 251)[n:]
    return out.reshape(img.shape)


def _top(npix):
    return 4097 if npix >= 4097 + 16 else npix - 600  # planted pixels; T3: 2472


def masked_terms(frame, layout, cfg, seed=5):
    """3 renders with the planted bin at top - 2, top - 1, top (T, T2: 4095 / 4096 / 4097) x warps whose masks give len_w = 1, 2, 3,
    4095, 4096, 4097, npix - 1, npix where the frame allows.  The small masks take texture pixels (a bin that is the whole of len
    has p = 1 and term 0 from any table); 4095 and 4097 take the planted zone first, so that counts of 4095 / 4096 meet
    len_w = 4097 and the count 4095 is all of len_w = 4095; the others keep the whole zone under a longer len."""
    w, h = FRAMES[frame]
    npix = w * h
    top = _top(npix)
    r, f, zone = _zone_pair(frame, top, seed, layout, cfg)
    rest = np.setdiff1d(np.arange(npix), zone)
    planted_first = np.concatenate([zone, rest])
    texture_first = np.concatenate([rest, zone])
    rs = np.stack([_with_zone(r, zone, top - 2 + k, seed + k) for k in range(3)])  # T: 4095, 4096, 4097
    lens, ws, wm = [], [], []
    for L, m255, order in ((1, top, texture_first), (2, top, texture_first), (3, top, texture_first), (4095, top, planted_first),
                           (4096, top, texture_first), (4097, top, planted_first), (npix - 1, top - 1, planted_first),
                           (npix, top, planted_first), (npix, top - 2, planted_first), (npix - 1, top - 1, texture_first)):
        if L > npix:
            continue
        lens.append(L)
        ws.append(_with_zone(f, zone, m255, seed + 10 + len(lens)))
        wm.append(_first(order, L, (h, w)))
    return dict(rs=rs, ws=np.stack(ws), wm=np.stack(wm), rm=np.ones_like(rs), cfg=dict(cfg), lens=lens, top=top)


COVER_LENS = {"T": (5120, 3, 4097, 0, 4096, 4095, 1), "T2": (4128, 3, 4097, 0, 4096, 4095, 1), "T3": (3072, 3, 3071, 0, 2600, 2473, 1)}


def covered_terms(frame, layout, cfg, seed=6):
    """4 warps x 7 renders whose masks give len[0][s] = COVER_LENS in the order one workgroup visits them without tiling
    (p = w * S + s ascending).  Warp 1 lacks one texture pixel and two planted ones, warp 2 three planted ones (a count of 4095 in
    ONE of the three histograms: where all three hold the same counts every term cancels out of the score), warp 3 one.  Large
    then small leaves entries above `top` stale.  On T and T2 the planted bin holds 4096 of len 5120 and of 4097 (evaluated
    inline), 4095 of 4096 (the table's last entry) and 4095 of 4095 (p = 1: every term is 0 and the score 0.0 unless a stale
    entry is read)."""
    w, h = FRAMES[frame]
    npix = w * h
    top = _top(npix)
    r, f, zone = _zone_pair(frame, top, seed, layout, cfg)
    rest = np.setdiff1d(np.arange(npix), zone)
    planted_first = np.concatenate([zone, rest])
    texture_first = np.concatenate([rest, zone])
    lens = COVER_LENS[frame]
    n255 = (top - 1, top, top - 1, top, top - 2, top, top)
    rs = np.stack([_with_zone(r, zone, n, seed + k) for k, n in enumerate(n255)])
    rm = np.stack([_first(texture_first if L <= 3 else planted_first, L, (h, w)) for L in lens])
    ws = np.stack([f] + [_with_zone(f, zone, top - k, seed + 18 + k) for k in (2, 3, 1)])
    wm = np.ones_like(ws)
    wm[1].reshape(-1)[rest[-1]] = 0  # warp 1: one texture pixel less where the render mask reaches it
    return dict(rs=rs, ws=ws, wm=wm, rm=rm, cfg=dict(cfg), lens=lens, top=top)


TERM_CFGS = {"bg": {}, "bgoff": dict(use_bg=False), "64bins": dict(bins=64), "enmi": dict(mode=oc.MODE_ENMI),
             "bgoff-enmi": dict(use_bg=False, mode=oc.MODE_ENMI), "64bins-enmi": dict(bins=64, mode=oc.MODE_ENMI)}
TERMS = {}
for _frame, _layout, _cfg in (("T", "scattered", "bg"), ("T", "runs", "bgoff"), ("T", "scattered", "64bins"), ("T", "runs", "enmi"),
                              ("T", "scattered", "bgoff-enmi"), ("T", "runs", "64bins-enmi"), ("T2", "scattered", "bg"),
                              ("T2", "runs", "bgoff"), ("T3", "scattered", "bg"), ("T3", "runs", "64bins")):
    TERMS[f"masked-{_frame}-{_cfg}-{_layout}"] = (masked_terms, _frame, _layout, _cfg)
    TERMS[f"covered-{_frame}-{_cfg}-{_layout}"] = (covered_terms, _frame, _layout, _cfg)


@functools.lru_cache(maxsize=None)
def terms(name):
    fn, frame, layout, cfg = TERMS[name]
    return fn(frame, layout, TERM_CFGS[cfg])


def masked_order(name="masked-T-bg-scattered"):
    """The 3 x 4 grid of the visiting-order test: warps of len_w 5120, 4096, 3 and 4097 (tables that differ in every entry)."""
    c = terms(name)
    pick = [7, 4, 2, 5]
    return dict(rs=c["rs"], ws=c["ws"][pick], wm=c["wm"][pick], rm=c["rm"], cfg=c["cfg"], lens=[c["lens"][k] for k in pick])


@functools.lru_cache(maxsize=None)
def cached_models(kind, name):
    return models({"case": case, "grid": grid, "terms": terms, "order": masked_order}[kind](name))
