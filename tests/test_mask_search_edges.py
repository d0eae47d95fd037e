"""Edge tests of the masked and covered GRID searches (csrc/nmi_masked_kernel.hip, csrc/nmi_covered_kernel.hip, csrc/nmi_mask_device.h)
on images whose joint histogram is controlled exactly (tests/helpers/wrap_cases.py).  Three mechanisms are these kernels' own:

1. the exact pixel form masked_add_chunk<.., HIST 1> (returning atomics in batches of four, the `any` selector, old = 0 for
   pixels that are not taken): one bin at exactly 65,535 / 65,536 / 65,537 hits of a low and of a high field, a low wrap whose
   carry wraps the high field, 131,071 / 131,072, a bin that passes 65,535 only if masked-out pixels were counted, a reduced bin
   made of four raw pairs, a wrap in row 0 / column 0 that is counted, detected and cleared, on the 16-byte and on the byte path;
2. the redo list between the optimistic and the exact launch: grids in which 0, 4 of 16, 6 of 30 or all candidates wrap, with
   1, 2, 3, 5 and the default number of workgroups, both visiting orders, a tie between two listed candidates, one context reused;
3. the terms: len_w and len on 1, 2, 3, 4095, 4096, 4097, npix - 1, npix, counts of 4095 / 4096 / 4097 either side of the LDS
   table, one workgroup that changes and keeps its warp, and a covered workgroup whose len shrinks and grows again.

Every GPU case runs through the masked and the covered search, each with default options (optimistic launch + redo) and with
NMI_OPT_HIST_VARIANT 1 (exact from the start).  The reference is masked_np.masked_search / covered_np.covered_search under
oracle.binding.rounded(); ratings, winner and score are compared with == on the bits, len_w and cover_counts with ==.  Every
grid has at most 32 candidates and must be a grid launch (pix_status).  On the two byte-path frames (ragged width, misaligned
stacks) the default routing sends so small a grid to the pixel-range kernels, which have tests of their own: there NMI_OPT_SPLIT 0
keeps the search on the grid kernels' byte path.

The unmarked tests run in the CPU tier and prove every premise: the planted counts are exact under the masks, exactly the
designed candidates fail the optimistic pass (wrap_cases.wraps), the len sequences and boundary counts are what the case names
say, and the rounded model agrees with an independent float64 score (wrap_cases.score_f64) to 4 x the largest difference seen."""
import numpy as np
import pytest

from helpers import wrap_cases as wc

gpu = pytest.mark.gpu
WORKGROUPS = (1, 2, 3, 5, 0)  # 0: the default, one per candidate up to the compute units


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def shift_of(cfg):
    return wc.SHIFT[cfg.get("bins", 256)]


# ======================================================================================================================================
# CPU tier: the helper, the premises of every case, the model against float64
# ======================================================================================================================================
@pytest.mark.parametrize("layout", ["scattered", "runs"])
def test_planted_counts_are_exact(layout):
    bins = [((9, 5), 700), ((9, 133), 1), ((0, 7), 33), ((200, 0), 64), ((255, 255), 5), ((17, 18), 0)]
    r, f = wc.planted(96, 43, bins, 3, layout)
    assert r.shape == f.shape == (43, 96) and r.dtype == f.dtype == np.uint8
    j = np.bincount(r.reshape(-1).astype(np.int64) * 256 + f.reshape(-1), minlength=65536).reshape(256, 256)
    for (d1, d2), n in bins:
        assert j[d1, d2] == n
    rest = np.ones((43, 96), bool)
    for (d1, d2), _ in bins:
        rest &= ~((r == d1) & (f == d2))
    assert rest.sum() == 96 * 43 - 803 and r[rest].min() >= 1 and r[rest].max() <= 254 and f[rest].min() >= 1 and f[rest].max() <= 254
    pos = np.flatnonzero((r == 9) & (f == 5))
    assert (np.ptp(pos) == 699) == (layout == "runs")  # contiguous, or not
    r2, f2 = wc.planted(96, 43, bins, 3, layout)
    assert np.array_equal(r, r2) and np.array_equal(f, f2)


def test_wraps_is_the_two_field_rule():
    def joint(**at):
        j = np.zeros((256, 256), np.int64)
        for k, v in at.items():
            j[9, int(k[1:])] = v
        return j
    assert not wc.wraps(joint(c5=65535)) and wc.wraps(joint(c5=65536)) and wc.wraps(joint(c5=131072))
    assert not wc.wraps(joint(c133=65535)) and wc.wraps(joint(c133=65536))
    assert not wc.wraps(joint(c5=65535, c133=65535))
    assert wc.wraps(joint(c5=65536, c133=65535)) and wc.wraps(joint(c5=65535, c133=65536))
    assert not wc.wraps(joint(c5=65535, c6=65535, c134=65535))  # neighbours are other words


@pytest.mark.parametrize("name", list(wc.CASES))
def test_field_case_premises(name):
    """The counted number of every planted pair is the table's under the masked and the covered masks; candidate (0, 0) fails the
    optimistic pass iff designed to, the three textured candidates never; len differs between the renders."""
    c, sp = wc.case(name), wc.CASES[name]
    w, h = wc.FRAMES[sp.frame]
    assert c["rs"].shape == c["ws"].shape == c["wm"].shape == c["rm"].shape == (2, h, w)
    extra = {"down": 5, "up": 100}.get(sp.mask, 0)
    d1, d2 = sp.pairs[0][0]
    assert ((c["rs"][0] == d1) & (c["ws"][0] == d2)).sum() == sp.pairs[0][1] + extra  # raw occurrences, masked-out ones included
    assert (c["wm"][0] == 0).sum() == 50 + extra and set(np.unique(c["wm"])) == ({0, 1, 2, 255} if sp.mask == "bytes" else {0, 1})
    raw_cfg = dict(c, cfg=dict(c["cfg"], bins=256))
    for covered in (False, True):
        j_raw = wc.hist(raw_cfg, 0, 0, covered, count_all=True)[0]
        for (p1, p2), n in sp.pairs:
            assert j_raw[p1, p2] == n, (name, covered, (p1, p2))
        if sp.cfg.get("bins") == 64:  # four raw pairs, one reduced bin
            j = wc.hist(c, 0, 0, covered)[0]
            want = sum(n for (p1, p2), n in sp.pairs if sp.cfg.get("use_bg", True) or (p1 and p2))
            assert len({(p1 >> 2, p2 >> 2) for (p1, p2), _ in sp.pairs}) == 1 and j[sp.pairs[0][0][0] >> 2, sp.pairs[0][0][1] >> 2] == want
        if not sp.cfg.get("use_bg", True) and sp.cfg.get("bins", 256) == 256:  # the wrapped bin is cleared afterwards
            assert d1 == 0 or d2 == 0
            assert wc.hist(c, 0, 0, covered)[0][d1, d2] == 0
        if wc.optimistic(sp.cfg):
            failing = [wc.wraps(wc.hist(c, v, s, covered, count_all=True)[0]) for v in range(2) for s in range(2)]
            assert failing == [sp.wraps, False, False, False], (name, covered)
    counts = wc.cached_models("case", name)[1][3]
    assert (counts[:, 0] != counts[:, 1]).all()


def test_field_case_table_covers_the_boundaries():
    names = set(wc.CASES)
    for n in (65535, 65536, 65537):
        for fld in ("lo", "hi"):
            for lay in ("scattered", "runs"):
                assert f"A-{fld}-{n}-{lay}" in names
    assert {wc.CASES[n].wraps for n in names if "-down-" in n} == {False} and {wc.CASES[n].wraps for n in names if "-up-" in n} == {True}
    assert {wc.CASES[n].frame for n in names} == {"A", "B", "R", "Amis"}
    assert wc.FRAMES["R"][0] % 16 != 0 and all(wc.FRAMES[f][0] % 16 == 0 for f in ("A", "B", "T", "T2", "T3"))
    assert all(w * h > 65536 for w, h in (wc.FRAMES[f] for f in ("A", "B", "R"))) and wc.FRAMES["T3"][0] * wc.FRAMES["T3"][1] < 4095


@pytest.mark.parametrize("name", list(wc.GRID_DEFS))
def test_redo_grid_premises(name):
    """Exactly the nearly-flat x nearly-flat candidates fail the optimistic pass, under both searches' masks; the winner is where
    the grid's name says."""
    g = wc.grid(name)
    (mr, mi, mb), (cr, ci, cb, cc) = wc.cached_models("grid", name)
    Wn, S = mr.shape
    assert Wn * S <= 32
    for covered in (False, True):
        failing = np.array([[wc.wraps(wc.hist(g, v, s, covered, count_all=True)[0]) for s in range(S)] for v in range(Wn)])
        assert np.array_equal(failing, g["flat"]) and failing.sum() == wc.GRID_WRAPS[name]
    listed = set(np.flatnonzero(g["flat"].reshape(-1)).tolist())
    for ratings, idx in ((mr, mi), (cr, ci)):
        if name == "4x4-winner-wraps":
            assert idx in listed
        if name == "4x4-winner-clean":
            assert idx not in listed
        if name == "4x4-tie":
            top = np.flatnonzero(bits(ratings).reshape(-1) == bits(ratings).reshape(-1)[idx]).tolist()
            assert top == [9, 11] and idx == 9 and set(top) <= listed and ratings.max() == ratings.reshape(-1)[idx]
    assert len(set(bits(mr).reshape(-1).tolist())) >= Wn * S // 2  # no constant table


@pytest.mark.parametrize("name", list(wc.TERMS))
def test_term_case_premises(name):
    c = wc.terms(name)
    covered = name.startswith("covered")
    w, h = wc.FRAMES[wc.TERMS[name][1]]
    npix, top = w * h, c["top"]
    b = 255 >> shift_of(c["cfg"])
    Wn, S = len(c["ws"]), len(c["rs"])
    assert Wn * S <= 32
    hs = {(v, s): wc.hist(c, v, s, covered) for v in range(Wn) for s in range(S)}
    assert not any(wc.wraps(wc.hist(c, v, s, covered, count_all=True)[0]) for v, s in hs)
    # the planted bin's count in the joint and in both marginals, where p < 1
    below = [[n for n, L in ((int(x[k][b, b] if k == 0 else x[k][b]), x[3]) for x in hs.values()) if n < L] for k in range(3)]
    if covered:
        counts = wc.cached_models("terms", name)[1][3]
        assert tuple(counts[0]) == c["lens"] == wc.COVER_LENS[wc.TERMS[name][1]]
        ratings = wc.cached_models("terms", name)[1][0]
        assert (counts[:, 3] == 0).all() and (ratings[:, 3] == 0).all() and (ratings[:, 2] != 0).any() and (ratings[:, 4] != 0).any()
        if npix >= 4097:
            assert c["lens"][1:] == (3, 4097, 0, 4096, 4095, 1) and c["lens"][0] == npix
            assert (ratings[[0, 1, 3], 5] == 0).all()  # (warps whose 255s fill it) one bin holds all of len = 4095: p = 1, every term 0
    else:
        assert [int(np.count_nonzero(m)) for m in c["wm"]] == c["lens"]
        assert c["lens"] == [L for L in (1, 2, 3, 4095, 4096, 4097, npix - 1, npix, npix, npix - 1) if L <= npix]
    if npix >= 4097:
        for k in range(3):  # joint, render marginal, frame marginal: counts either side of the table under a longer len
            assert {4095, 4096}.issubset(below[k]) and (covered or 4097 in below[k]), (k, sorted(set(below[k])))
    else:
        assert npix < 4095 and max(x[3] for x in hs.values()) == npix


def test_masked_order_premises():
    g = wc.masked_order()
    assert g["lens"] == [5120, 4096, 3, 4097] and g["rs"].shape[0] == 3


F64_NAMES = [("case", n) for n in wc.CASES] + [("terms", n) for n in wc.TERMS]


@pytest.mark.parametrize("kind,name", F64_NAMES, ids=[n for _, n in F64_NAMES])
def test_model_agrees_with_float64(kind, name):
    """The rounded model against wrap_cases.score_f64, written here from the count rule alone (len, the background rule, the
    shift): a shared misreading of that rule would move a score by far more than fp32 rounding does."""
    c = wc.case(name) if kind == "case" else wc.terms(name)
    (mr, _, _), (cr, _, _, _) = wc.cached_models(kind, name)
    worst = max(float(np.abs(mr - wc.f64_table(c, False)).max()), float(np.abs(cr - wc.f64_table(c, True)).max()))
    print(f"{name}: max |model - f64| = {worst:.3g}")
    assert worst <= 4 * wc.F64_SEEN


# ======================================================================================================================================
# GPU tier
# ======================================================================================================================================
@pytest.fixture(scope="module")
def device():
    import torch
    from orbslam2_nmi_amd import capi
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    capi.load_library()  # raises if the HIP library is missing: there is no fallback
    return capi


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def search(ctx, covered, d, shape, want, what):
    """One search on `ctx` of the device stacks d = (rs, ws, wm, rm) against the model `want`; must be a grid launch."""
    import torch
    Wn, S = shape
    ratings = torch.full((Wn, S), -7.0, dtype=torch.float32, device="cuda")
    if covered:
        idx, best = ctx.search_grid_covered(d[0], d[3], d[1], d[2], ratings)
    else:
        idx, best = ctx.search_grid_masked(d[0], d[1], d[2], ratings)
    assert ctx.pix_status()["last_launch_ranges"] == 0 and ctx.split_status()["last_launch_parts"] == 0, what  # the grid form
    got = ratings.cpu().numpy()
    bad = np.argwhere(bits(got) != bits(want[0]))
    assert bad.size == 0, (what, bad[:5].tolist(), got[tuple(bad[0])], want[0][tuple(bad[0])])
    assert (idx, int(bits(best)[0])) == (want[1], int(bits(want[2])[0])), (what, idx, best, want[1], want[2])
    if covered:
        assert np.array_equal(ctx.cover_counts(Wn * S).reshape(Wn, S), want[3]), what
    else:
        assert np.array_equal(ctx.mask_counts(Wn), np.count_nonzero(d[2].cpu().numpy().reshape(Wn, -1), axis=1)), what


def four_ways(capi, c, want, options=None, place=dev):
    """Masked and covered search, each with default options and exact from the start; a fresh context each."""
    N = capi.NmiContext
    rs, ws, wm, rm = wc.stacks(c)
    d = tuple(place(a) for a in (rs, ws, wm, rm))
    h, w = rs.shape[1:]
    cfg = c["cfg"]
    for covered in (False, True):
        for exact in (False, True):
            opts = dict(options or {})
            if exact:
                opts[N.OPT_HIST_VARIANT] = 1
            with N(w, h, bins=cfg.get("bins", 256), mode=cfg.get("mode", capi.MODE_SUC), use_bg=cfg.get("use_bg", True),
                   render_bottom_up=cfg.get("bottom_up", True)) as ctx:
                for k, v in opts.items():
                    ctx.set_option(k, v)
                search(ctx, covered, d, (len(ws), len(rs)), want[1 if covered else 0], ("covered" if covered else "masked", opts))


@gpu
@pytest.mark.parametrize("name", list(wc.CASES))
def test_field_boundaries(device, name):
    capi = device
    sp = wc.CASES[name]
    options, place = {}, dev
    if sp.frame in wc.BYTE_PATH:
        options = {capi.NmiContext.OPT_SPLIT: 0}  # stay on the grid kernels' byte path (see the module docstring)
    if sp.frame == "Amis":
        from test_masked_search import misaligned
        place = misaligned
    four_ways(capi, wc.case(name), wc.cached_models("case", name), options, place)


@gpu
@pytest.mark.parametrize("workgroups", WORKGROUPS)
@pytest.mark.parametrize("name", [n for n in wc.GRID_DEFS if n != "5x6"])
def test_redo_list(device, name, workgroups):
    """1 workgroup: wrapped and clean candidates in turn, and an exact launch that strides a list longer than its grid; 5 and more:
    workgroups of the exact launch that find nothing.  Both visiting orders."""
    capi = device
    N = capi.NmiContext
    for tiling in (1, 0):
        opts = {N.OPT_XCD_TILING: tiling}
        if workgroups:
            opts[N.OPT_WORKGROUPS] = workgroups
        four_ways(capi, wc.grid(name), wc.cached_models("grid", name), opts)


@gpu
def test_redo_list_reuse(device):
    """One context, one pass: 4 of 16 on the list, none, all 9, the covered search of the same stacks (it shares the list), then a
    5 x 6 grid for which the list grows."""
    capi = device
    w, h = wc.FRAMES["A"]
    with capi.NmiContext(w, h) as ctx:
        for step, name in enumerate(wc.REUSE_ORDER):
            g = wc.grid(name)
            rs, ws, wm, rm = wc.stacks(g)
            d = tuple(dev(a) for a in (rs, ws, wm, rm))
            want = wc.cached_models("grid", name)
            search(ctx, False, d, (len(ws), len(rs)), want[0], (step, name, "masked"))
            if step >= 2:
                search(ctx, True, d, (len(ws), len(rs)), want[1], (step, name, "covered"))


@gpu
@pytest.mark.parametrize("name", list(wc.TERMS))
def test_terms(device, name):
    """Default workgroups, and one workgroup without tiling: p = w * S + s ascending, the len order of the covered cases."""
    capi = device
    N = capi.NmiContext
    c, want = wc.terms(name), wc.cached_models("terms", name)
    four_ways(capi, c, want)
    four_ways(capi, c, want, {N.OPT_WORKGROUPS: 1, N.OPT_XCD_TILING: 0})
    four_ways(capi, c, want, {N.OPT_WORKGROUPS: 1, N.OPT_XCD_TILING: 1})


@gpu
@pytest.mark.parametrize("workgroups", [1, 5])
@pytest.mark.parametrize("tiling", [1, 0])
def test_masked_visiting_order(device, workgroups, tiling):
    """3 x 4 grid whose four warps have tables that differ in every entry.  One workgroup changes its warp (reload) and keeps it (no
    reload) within one launch; with 5 workgroups and no tiling workgroup 3 starts at candidate 3 = warp 1, workgroup 4 at warp 1 too,
    so a workgroup's first table is not warp 0's."""
    capi = device
    N = capi.NmiContext
    g = wc.masked_order()
    four_ways(capi, g, wc.cached_models("order", "masked-T-bg-scattered"), {N.OPT_WORKGROUPS: workgroups, N.OPT_XCD_TILING: tiling})
