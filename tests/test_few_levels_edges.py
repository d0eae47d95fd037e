"""Edge tests of the few-levels path (csrc/nmi_fewlevels_kernel.hip: probe, rank images, scoring kernel; routed by enqueue_grid in
csrc/nmi_capi.cpp) on stacks whose level sets are controlled exactly (tests/helpers/level_cases.py).  The content of the images
decides the rank tables, the nr x nw joint histogram, the number of interleaved counter copies (32 / 16 / 8), the row and column
the background rule clears and whether the search is handed back to the gated general kernel -- so the cases sit on those edges:
joint sizes either side of every copy-count switch and of the 4096 limit, levels on the first and last bits of the presence
words, a level that occurs in ONE pixel at the places where the probe can lose a chunk, frames with fewer chunks than lanes and
with a second trip of the probe loop, shards at non-zero offsets, several candidates per workgroup in both visiting orders, and the
general kernel acting as the content probe (LevelPlan::seen) with exact counts.

The reference is the CPU oracle in its rounded term mode; every rating is compared as uint32 bits with ==, winner and score with
==; level counts from last_content() with == (the probe of a few-levels launch is exact).  No tolerance anywhere.

The unmarked tests run in the CPU tier: they check the helper (every stack holds exactly the set it was asked for), that every
planted-pixel case is SENSITIVE (merging the planted level with its neighbour, or with the stack's lowest level -- what a missed
presence bit does -- changes the bits of every rating the planted image takes part in), that the exact-joint cases do not have
constant rating tables, and that the probe cases reach every bit of every seen[] word."""
import functools

import numpy as np
import pytest

from helpers import level_cases as lc

gpu = pytest.mark.gpu
W, H = lc.W, lc.H
SHIFT = {256: 0, 64: 2, 16: 4}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def oracle(rs, ws, **kw):
    from oracle import binding as oc
    with oc.rounded():
        return oc.search_grid(rs, ws, threads=16, **kw)


@functools.lru_cache(maxsize=None)
def joint_want(name):
    rs, ws = lc.joint_stacks(name)
    return rs, ws, oracle(rs, ws)


@functools.lru_cache(maxsize=None)
def grid27_want():
    rs, ws = lc.grid27_stacks()
    return rs, ws, oracle(rs, ws)


def plant_groups():
    return [(w, h, bu, which) for (w, h) in lc.PLANT_FRAMES for bu in (True, False) for which in (0, 1)]


# ======================================================================================================================================
# CPU tier: the helper and the case tables
# ======================================================================================================================================
def same_set(stack, levels, shift=0):
    return np.array_equal(np.unique(stack >> shift), np.unique(np.asarray(levels, np.uint8)))


def test_exact_levels_and_plant():
    rng = np.random.default_rng(1)
    for levels in [(0,), (255,), (0, 255), tuple(range(256)), lc.BOUNDARY]:
        for shape in [(1, 1, 256), (2, 16, 16), (9, H, W)]:
            assert same_set(lc.exact_levels(shape, levels, rng), levels)
    s = lc.exact_levels((2, 3, 48), (5, 9), rng)
    p = lc.plant(s, 1, 47, 7)
    assert p[1].reshape(-1)[47] == 7 and (p == 7).sum() == 1 and (p != s).sum() == 1 and not (s == 7).any()
    with pytest.raises(AssertionError):
        lc.plant(s, 0, 0, 9)  # 9 is there already


@pytest.mark.parametrize("name", list(lc.JOINT_CASES))
def test_joint_cases_are_exact_and_not_degenerate(name):
    """np.unique of both stacks == the requested sets (so nr x nw is the joint size in the name), and the 81 oracle ratings are
    not all equal -- except where one stack is constant: those are all 0 by construction (the all-zero guard)."""
    r, w, _ = lc.JOINT_CASES[name]
    rs, ws, (ro, _, _) = joint_want(name)
    assert same_set(rs, r) and same_set(ws, w)
    if name[0].isdigit():
        assert (len(r), len(w)) == tuple(int(v) for v in name.split("x"))
    if name in lc.ALL_ZERO_JOINTS:
        assert (ro == 0).all()
    else:
        assert len(set(bits(ro).reshape(-1).tolist())) == 81, name


def test_joint_sizes_sit_on_the_copy_count_edges():
    size = {n: len(r) * len(w) for n, (r, w, _) in lc.JOINT_CASES.items()}
    assert [size[n] for n in ("32x32", "25x41", "64x32", "41x50", "64x64", "256x16", "16x256", "17x241", "256x1", "1x256", "1x1")] == \
        [1024, 1025, 2048, 2050, 4096, 4096, 4096, 4097, 256, 256, 1]
    assert all(few == (size[n] <= 4096) for n, (_, _, few) in lc.JOINT_CASES.items())
    assert all(taken == (size[n] <= limit) and size[n] - limit in (0, 1) for n, limit, taken in lc.LIMIT_CASES)


def test_other_case_tables_are_exact():
    r, w = lc.ABSENT_SETS
    rs, ws = lc.absent_stacks()
    assert same_set(rs, r) and same_set(ws, w)
    for i in range(9):  # every image: its own half, so rows / columns between occupied ones are empty
        assert same_set(rs[i], r[i % 2::2]) and same_set(ws[i], w[i % 2::2])
    for name, (r, w) in lc.ZERO_CASES.items():
        rs, ws = lc.zero_stacks(name)
        assert same_set(rs, r) and same_set(ws, w), name
    assert [(0 in r, 0 in w) for r, w in lc.ZERO_CASES.values()] == [(True, True), (True, False), (False, True), (False, False), (True, True)]
    rs, ws = lc.zero_stacks("late0")
    assert not (rs[0] == 0).any() and not (ws[0] == 0).any() and (rs[1:] == 0).any() and (ws[1:] == 0).any()
    for bins, nrb, nwb in lc.BIN_CASES:
        rb, wb, rr, wr = lc.bin_sets(bins, nrb, nwb)
        rs, ws = lc.bin_stacks(bins, nrb, nwb)
        assert (len(rb), len(wb)) == (nrb, nwb) and same_set(rs, rr) and same_set(ws, wr)
        assert same_set(rs, rb, SHIFT[bins]) and same_set(ws, wb, SHIFT[bins])
        for raw, b in ((rr, rb), (wr, wb)):  # raw values differ inside every bin: counting values instead of bins shows
            assert all(sum(1 for v in raw if v >> SHIFT[bins] == x) >= 2 for x in b)
    rs, ws = lc.hot_stacks()
    assert same_set(rs, (77, 130)) and same_set(ws, (9, 201)) and (rs == 130).sum() == 1 and (ws == 9).sum() == 1
    rs, ws = lc.grid27_stacks()
    assert same_set(rs, lc.GRID27_SETS[0]) and same_set(ws, lc.GRID27_SETS[1]) and same_set(rs[:lc.GRID27_FIRST], lc.GRID27_SETS[0][:4])
    assert [a for a, _ in lc.RENDER_SHARDS[1:]] == [3, 9, 18] and lc.RENDER_SHARDS[-1][1] == 27 and lc.WARP_SHARDS[-1][1] == 27
    (a, b), ((ars, aws), (brs, bws)) = lc.changing_sets(), lc.changing_stacks()
    assert same_set(ars, a[0]) and same_set(aws, a[1]) and same_set(brs, b[0]) and same_set(bws, b[1])
    assert (len(a[0]), len(a[1]), len(b[0]), len(b[1])) == (40, 50, 3, 2)
    assert not set(b[0]) & set(a[0]) and not set(b[1]) & set(a[1])
    for name, (bins, r, w) in lc.PROBE_CASES.items():
        rs, ws = lc.probe_stacks(name)
        assert same_set(rs, r) and same_set(ws, w)
        nr, nw = lc.probe_counts(name)
        assert (nr, nw) == (len(np.unique(rs >> SHIFT[bins])), len(np.unique(ws >> SHIFT[bins]))) and nr * nw >= 2
    (frs, fws), (mrs, mws) = lc.verdict_stacks()
    assert len(np.unique(frs)) * len(np.unique(fws)) * 2 <= 4096 and len(np.unique(mrs)) * len(np.unique(mws)) >= 2 * 4096


def test_plant_positions_reach_the_probes_edges():
    """The positions named by the frames' table: slices with no chunk at all (32 x 1), chunks per row that do not divide into the
    slices (48 x 3), and a slice of 4097 chunks = one trip of 4 x 1024 loads and a second one whose last three loads are clamped."""
    assert lc.probe_slice_chunks(32) == (2, 1) and lc.plant_positions(32, 1) == [0, 15, 16, 31]
    assert lc.probe_slice_chunks(48 * 3) == (9, 3) and lc.plant_positions(48, 3) == [0, 15, 16, 47, 48, 95, 96, 128, 143]
    n, per = lc.probe_slice_chunks(64 * 4097)
    assert (n, per) == (4 * 4097, 4097) and per == lc.PROBE_BLOCK * lc.PROBE_LOADS + 1
    pos = lc.plant_positions(64, 4097)
    assert len(pos) == 11 and all(16 * k * per - 1 in pos and 16 * k * per in pos for k in (1, 2, 3))
    assert lc.flipped(0, 48, 3) == 96 and lc.flipped(143, 48, 3) == 47 and lc.flipped(50, 48, 3) == 50
    for w, h, bu, which in plant_groups():
        cases = lc.plant_cases(w, h, bu, which)
        assert len(set(cases)) == len(cases) and (1, w * h - 1) in cases and (1, (w * h // 16 - 1) * 16) in cases
        assert {p for _, p in cases} >= set(lc.plant_positions(w, h))
        if bu and which == 0:
            assert {p for _, p in cases} >= {lc.flipped(p, w, h) for p in lc.plant_positions(w, h)}


@pytest.mark.parametrize("w,h,bottom_up,which", plant_groups())
def test_every_planted_pixel_is_sensitive(w, h, bottom_up, which):
    """No planted-pixel case can pass vacuously: with the planted value replaced by the nearest level of its stack (two ranks
    merged) and by the stack's lowest level (rank 0 is what an absent intensity maps to: a missed presence bit), the oracle's
    bits change for BOTH candidates of the planted image, at every position."""
    base = lc.PLANT_SETS[which]
    value = lc.PLANT_VALUE[which]
    assert value not in base and min(base) < value < max(base)
    for image, pos in lc.plant_cases(w, h, bottom_up, which):
        rs, ws = lc.planted(w, h, which, image, pos)
        assert same_set(rs, lc.PLANT_SETS[0] + ((value,) if which == 0 else ())) and same_set(ws, lc.PLANT_SETS[1] + ((value,) if which == 1 else ()))
        ro, _, _ = oracle(rs, ws, render_bottom_up=bottom_up)
        for other in (lc.nearest_level(base, value), min(base)):
            stacks = [rs.copy(), ws.copy()]
            assert stacks[which][image].reshape(-1)[pos] == value
            stacks[which][image].reshape(-1)[pos] = other
            alt, _, _ = oracle(stacks[0], stacks[1], render_bottom_up=bottom_up)
            changed = bits(alt) != bits(ro)  # [warp, render]
            involved = changed[:, image] if which == 0 else changed[image, :]
            assert involved.all(), (w, h, bottom_up, which, image, pos, other)


def test_probe_cases_reach_every_bit_of_every_seen_word():
    """LevelPlan::seen: 16 words per stack, bit k of word i = bin i + 16 k below 128, i + 16 (k - 8) + 128 above.  The eight
    partition pairs hold every intensity on each side, i.e. all 16 bits of all 32 words."""
    assert sorted(lc.seen_slot(b) for b in range(256)) == [(i, k) for i in range(16) for k in range(16)]
    assert lc.seen_slot(0) == (0, 0) and lc.seen_slot(127) == (15, 7) and lc.seen_slot(128) == (0, 8) and lc.seen_slot(255) == (15, 15)
    assert lc.seen_slot(17) == (1, 1) and lc.seen_slot(17 + 128) == (1, 9)
    for side in (0, 1):
        held = [v for pair in lc.PARTITION_SETS for v in pair[side]]
        assert sorted(held) == list(range(256))
        assert {lc.seen_slot(v) for v in held} == {(i, k) for i in range(16) for k in range(16)}
    assert all(lc.probe_counts(f"partition{i}") == (32, 32) for i in range(8))


# ======================================================================================================================================
# GPU tier
# ======================================================================================================================================
@pytest.fixture(scope="module")
def nmi():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    import orbslam2_nmi_amd as m
    m.load_library()
    return m


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def context(nmi, w=W, h=H, path=1, split=None, workgroups=None, tiling=None, limit=None, **kw):
    ctx = nmi.NmiContext(w, h, **kw)
    ctx.set_option(ctx.OPT_CONTENT_PATH, path)
    for opt, val in ((ctx.OPT_SPLIT, split), (ctx.OPT_WORKGROUPS, workgroups), (ctx.OPT_XCD_TILING, tiling), (ctx.OPT_FEWLEVELS_BINS, limit)):
        if val is not None:
            ctx.set_option(opt, val)
    return ctx


def search(ctx, rs, ws, want):
    """One blocking search; ratings, winner and score must equal the oracle's `want`.  -> last_content()."""
    import torch
    ro, io, bo = want
    ratings = torch.full((ws.shape[0], rs.shape[0]), -7.0, dtype=torch.float32, device="cuda")
    idx, best = ctx.search_grid(dev(rs), dev(ws), ratings)
    info = ctx.last_content()
    r = ratings.cpu().numpy()
    assert (bits(r) == bits(ro)).all(), (int((bits(r) != bits(ro)).sum()), float(np.abs(r - ro).max()), info)
    assert (idx, best) == (io, bo), (idx, best, io, bo, info)
    return info


def grid_kernel_ran(ctx):
    return ctx.split_status()["last_launch_parts"] == 0 and ctx.pix_status()["last_launch_ranges"] == 0


def content(few, nr, nw):
    return {"few_levels": few, "nr": nr, "nw": nw}


# ---- section 2: the few-levels path forced -----------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", list(lc.JOINT_CASES))
def test_exact_joint_sizes(nmi, name):
    """1024 (the last size with 32 copies) / 1025, 2048 (16) / 2050 (8), 4096 in three shapes (taken), 4097 (handed back on the
    device, same bits), one constant stack, 1 x 1, and sets on the first and last bits of the presence words."""
    r, w, few = lc.JOINT_CASES[name]
    rs, ws, want = joint_want(name)
    with context(nmi) as ctx:
        assert search(ctx, rs, ws, want) == content(few, len(r), len(w))
        assert search(ctx, rs, ws, want) == content(few, len(r), len(w))  # and again on the plan the first search left


@gpu
@pytest.mark.parametrize("name,limit,taken", lc.LIMIT_CASES)
def test_limit_is_inclusive(nmi, name, limit, taken):
    """NMI_OPT_FEWLEVELS_BINS = L: a joint of exactly L is taken, L + 1 is handed back.  Both kernels give the same bits, so
    what tells them apart is last_content()'s few_levels: the verdict the probe left on the device (LevelPlan::use), read back."""
    r, w, _ = lc.JOINT_CASES[name]
    rs, ws, want = joint_want(name)
    with context(nmi, limit=limit) as ctx:
        assert search(ctx, rs, ws, want) == content(taken, len(r), len(w))


@gpu
def test_levels_absent_from_an_image(nmi):
    """Every image uses half of its stack's levels: zero rows and columns between occupied ones in every candidate's joint."""
    rs, ws = lc.absent_stacks()
    with context(nmi) as ctx:
        assert search(ctx, rs, ws, oracle(rs, ws)) == content(True, len(lc.ABSENT_SETS[0]), len(lc.ABSENT_SETS[1]))


@gpu
@pytest.mark.parametrize("name", list(lc.ZERO_CASES))
def test_background_rule_off(nmi, name):
    """Intensity 0 in both stacks, in one only (the other's lowest level is not 0: its rank 0 must stay), in neither, and in the
    stack but not in image 0; both score forms, both row orders."""
    r, w = lc.ZERO_CASES[name]
    rs, ws = lc.zero_stacks(name)
    for mode in (0, 1):
        for bottom_up in (True, False):
            want = oracle(rs, ws, use_bg=False, mode=mode, render_bottom_up=bottom_up)
            with context(nmi, use_bg=False, mode=mode, render_bottom_up=bottom_up) as ctx:
                assert search(ctx, rs, ws, want) == content(True, len(r), len(w)), (mode, bottom_up)


@gpu
@pytest.mark.parametrize("bins,nrb,nwb", lc.BIN_CASES)
def test_reduced_bins_count_bins_not_values(nmi, bins, nrb, nwb):
    """64 and 16 bins with the rule on: several raw values inside every bin, nr and nw count bins."""
    rs, ws = lc.bin_stacks(bins, nrb, nwb)
    with context(nmi, bins=bins) as ctx:
        assert search(ctx, rs, ws, oracle(rs, ws, shift=SHIFT[bins])) == content(True, nrb, nwb)


@gpu
@pytest.mark.parametrize("w,h,bottom_up,which", plant_groups())
def test_one_planted_pixel(nmi, w, h, bottom_up, which):
    """A level that occurs in ONE pixel of the stack (test_every_planted_pixel_is_sensitive: losing or merging it changes both
    ratings of its image): first byte, bytes 15 and 16, last byte, last chunk, either side of every slice boundary of the probe;
    2 x 2 candidates by the few-levels kernel (split forms off)."""
    nr, nw = len(lc.PLANT_SETS[0]) + (which == 0), len(lc.PLANT_SETS[1]) + (which == 1)
    with context(nmi, w, h, split=0, render_bottom_up=bottom_up) as ctx:
        for image, pos in lc.plant_cases(w, h, bottom_up, which):
            rs, ws = lc.planted(w, h, which, image, pos)
            info = search(ctx, rs, ws, oracle(rs, ws, render_bottom_up=bottom_up))
            assert info == content(True, nr, nw), (image, pos, info)
            assert ctx.split_status()["last_launch_parts"] == 0


@gpu
def test_hot_bin(nmi):
    """640 x 480, constant stacks but for one pixel each: 307,199 hits in one bin across the copies, table read at npix - 1 (and,
    for the pair of untouched images, 307,200 and table[npix])."""
    rs, ws = lc.hot_stacks()
    with context(nmi, 640, 480, split=0) as ctx:
        assert search(ctx, rs, ws, oracle(rs, ws)) == content(True, 2, 2)


@gpu
@pytest.mark.parametrize("workgroups", [8, 5, None])
@pytest.mark.parametrize("tiling", [0, 1])
def test_candidates_per_workgroup_and_visiting_order(nmi, workgroups, tiling):
    """729 candidates on 8 workgroups (a multiple of 8: slot_in_round's first branch, 91 or 92 candidates each), on 5 (its
    second branch) and on the default number; candidate order as it comes and XCD-tiled."""
    rs, ws, want = grid27_want()
    with context(nmi, workgroups=workgroups, tiling=tiling) as ctx:
        assert search(ctx, rs, ws, want) == content(True, 6, 5)


@gpu
@pytest.mark.parametrize("blocking", [True, False])
def test_shards_at_offsets(nmi, blocking):
    """The 27 x 27 search cut along the render axis (s_offset 3, 9, 18 after the first shard) and along the warp axis (w_offset):
    every shard's table == that slice of the oracle's, max of the keys == the oracle's winner.  Renders 0..2 hold four of the six
    levels: that shard's counts are its own."""
    import torch
    rs, ws, (ro, io, bo) = grid27_want()
    drs, dws = dev(rs), dev(ws)
    with context(nmi) as ctx:
        for axis, shards in ((1, lc.RENDER_SHARDS), (0, lc.WARP_SHARDS)):
            keys, tabs = [], []
            for a, b in shards:
                key = torch.zeros(1, dtype=torch.int64, device="cuda")
                if axis == 1:
                    t = torch.full((27, b - a), -7.0, dtype=torch.float32, device="cuda")
                    k = ctx.search_grid_shard(drs[a:b].contiguous(), a, 27, dws, ratings=t, key_out=key, blocking=blocking)
                    levels = len(np.unique(rs[a:b]))
                    assert levels == (4 if b <= lc.GRID27_FIRST else 6)
                    assert ctx.last_content() == content(True, levels, 5), (a, b)
                else:
                    t = torch.full((b - a, 27), -7.0, dtype=torch.float32, device="cuda")
                    k = ctx.search_grid_shard(drs, 0, 27, dws[a:b].contiguous(), ratings=t, key_out=key, blocking=blocking, w_offset=a, wn_total=27)
                    assert ctx.last_content() == content(True, 6, 5), (a, b)
                dk = int(key.cpu().numpy().view(np.uint64)[0])
                assert k is None or k == dk
                keys.append(dk)
                tabs.append(t.cpu().numpy())
            for (a, b), t in zip(shards, tabs):
                part = ro[:, a:b] if axis == 1 else ro[a:b]
                assert (bits(t) == bits(part)).all(), (axis, a, b)
            assert nmi.key_unpack(max(keys)) == (io, bo), axis


@gpu
def test_non_blocking_shards_back_to_back(nmi):
    """The same shards enqueued without a host wait between them (one plan, one pair of rank buffers, reused by every launch)."""
    import torch
    rs, ws, (ro, io, bo) = grid27_want()
    drs, dws = dev(rs), dev(ws)
    with context(nmi) as ctx:
        keys = [torch.zeros(1, dtype=torch.int64, device="cuda") for _ in lc.RENDER_SHARDS]
        tabs = [torch.full((27, b - a), -7.0, dtype=torch.float32, device="cuda") for a, b in lc.RENDER_SHARDS]
        parts = [drs[a:b].contiguous() for a, b in lc.RENDER_SHARDS]
        for (a, b), p, k, t in zip(lc.RENDER_SHARDS, parts, keys, tabs):
            ctx.search_grid_shard(p, a, 27, dws, ratings=t, key_out=k, blocking=False)
        ctx.synchronize()
        assert ctx.last_content() == content(True, 6, 5)
        for (a, b), t in zip(lc.RENDER_SHARDS, tabs):
            assert (bits(t.cpu().numpy()) == bits(ro[:, a:b])).all(), (a, b)
        assert nmi.key_unpack(max(int(k.cpu().numpy().view(np.uint64)[0]) for k in keys)) == (io, bo)


@gpu
def test_one_context_changing_sets(nmi):
    """A (40 x 50 levels), B (3 x 2, none of them A's), A again: level_r / level_w entries beyond the new nr / nw are stale and
    must not leak into the rank tables."""
    (ars, aws), (brs, bws) = lc.changing_stacks()
    wa, wb = oracle(ars, aws), oracle(brs, bws)
    with context(nmi) as ctx:
        assert search(ctx, ars, aws, wa) == content(True, 40, 50)
        assert search(ctx, brs, bws, wb) == content(True, 3, 2)
        assert search(ctx, ars, aws, wa) == content(True, 40, 50)
        assert search(ctx, brs, bws, wb) == content(True, 3, 2)


# ---- section 3: the general kernel as probe ------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", list(lc.PROBE_CASES))
def test_general_kernel_counts_exactly_through_the_verdict_change(nmi, name):
    """Automatic mode, ONE workgroup (its ORs into LevelPlan::seen and the final exchange come from one wavefront, in order), 3 x 3
    candidates by nmi_grid_kernel.  Limit = nr * nw: search 1 is general and posts the exact counts, search 2 takes the few-levels
    path.  Limit = nr * nw - 1: the verdict does not change, nothing is posted, search 2 is general again."""
    bins = lc.PROBE_CASES[name][0]
    nr, nw = lc.probe_counts(name)
    rs, ws = lc.probe_stacks(name)
    want = oracle(rs, ws, shift=SHIFT[bins])
    with context(nmi, path=-1, workgroups=1, limit=nr * nw, bins=bins) as ctx:
        assert search(ctx, rs, ws, want) == content(False, nr, nw)
        assert grid_kernel_ran(ctx)
        assert search(ctx, rs, ws, want) == content(True, nr, nw)
        assert search(ctx, rs, ws, want) == content(True, nr, nw)
    with context(nmi, path=-1, workgroups=1, limit=nr * nw - 1, bins=bins) as ctx:
        for _ in range(2):
            assert search(ctx, rs, ws, want) == content(False, 0, 0)
            assert grid_kernel_ran(ctx)


@gpu
def test_default_workgroups_follow_the_content(nmi):
    """144 candidates on the default number of workgroups: nmi_grid_kernel is the probe (81 candidates, as in
    test_few_levels.py, are the pixel-range kernel's).  Counts of a multi-workgroup launch are a hint (finish_search), so the
    content is a factor of two away from the limit on either side and only the verdicts are asserted."""
    few, many = lc.verdict_stacks()
    want = {id(few): oracle(*few), id(many): oracle(*many)}
    seq = [(few, False, True), (few, True, False), (few, True, False), (many, False, False), (many, False, True), (few, False, True), (few, True, False)]
    with context(nmi, path=-1) as ctx:
        for k, (stacks, is_few, general) in enumerate(seq):
            info = search(ctx, *stacks, want[id(stacks)])
            assert info["few_levels"] == is_few, (k, info)
            if general:
                assert grid_kernel_ran(ctx), k
