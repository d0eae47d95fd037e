"""GPU parity tests (-m gpu): the HIP path, called through the C ABI, against the CPU oracle on identical inputs.

Bars: integer work (joint / marginal histograms, arg-max index) bit-exact.  Floating point: against the oracle in its
"rounded" term mode (oracle/nmi_oracle.c nmi_oracle_bin_term: the fp64 log2 rounded once to fp32 -- the same value the
product's per-count table holds, checked entry by entry in test_term_table_equals_oracle) every entropy sum, every
rating and every winner is compared with ==: same fp32 operations in the reference's order (NMI.cu:270-339).  Against
the oracle's libm mode (the expression as written, log2f of this host) the north_star's 1e-5 is kept as a cross-check.
The oracle is "parity unpinned" against the reference's CUDA kernels (no golden vectors exist there and they cannot be
built here, oracle/nmi_oracle.c header); the analytic known answers are checked on the GPU directly as well."""
import time

import numpy as np
import pytest

from conftest import dense_joint

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SCORE_TOL = 1e-5  # north_star: "within 1e-5" -- only for comparisons with the libm-mode oracle and stored fixtures
SUM_TOL = 2e-6


@pytest.fixture(scope="module")
def nmi():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    import orbslam2_nmi_amd as m
    m.load_library()  # raises if the HIP library is missing: there is no fallback
    return m


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# Kernel selection for small grids (NMI_OPT_SPLIT): -1 automatic (K = 8 / 4 / 2 workgroups per candidate when the grid
# leaves compute units idle), 0 the one-workgroup-per-candidate kernel only, 8 / 4 / 2 forced.  Tests that take this
# fixture run once per mode; results must be identical bit for bit.
# A tuple (8, P) additionally forces P pixel ranges per row part (NMI_OPT_SPLIT_PIXELS); plain 8 / 4 / 2 run without them.
# (1, P): no row parts, P pixel ranges per candidate -- nmi_pix_kernel, the form of mid-size grids (csrc/nmi_pix_kernel.hip).
@pytest.fixture(params=[-1, 0, (8, 4), (8, 2), (4, 2), 8, 4, 2, (1, 2), (1, 3), (1, 4)],
                ids=lambda m: {-1: "auto", 0: "nosplit"}.get(m, f"split{m[0]}x{m[1]}" if isinstance(m, tuple) else f"split{m}"))
def split_mode(request, nmi):
    from orbslam2_nmi_amd import capi
    m = request.param
    C = capi.NmiContext
    if isinstance(m, tuple):
        C.default_options = {C.OPT_SPLIT: m[0], C.OPT_SPLIT_PIXELS: m[1]}
    elif m == -1:
        C.default_options = {C.OPT_SPLIT: -1}
    else:
        C.default_options = {C.OPT_SPLIT: m, C.OPT_SPLIT_PIXELS: 1}
    yield m
    C.default_options = {}


@pytest.fixture(params=[-1, 0], ids=["auto", "nosplit"])
def split_mode2(request, nmi):
    from orbslam2_nmi_amd import capi
    capi.NmiContext.default_options = {capi.NmiContext.OPT_SPLIT: request.param}
    yield request.param
    capi.NmiContext.default_options = {}


def check_pair(nmi, oc, r, w, bins=256, mode=1, bg=True, bu=True):
    h, wd = r.shape
    shift = {256: 0, 128: 1, 64: 2, 32: 3, 16: 4}[bins]
    with nmi.NmiContext(wd, h, bins=bins, mode=mode, use_bg=bg, render_bottom_up=bu) as ctx:
        s, j, h1, h2, sums = ctx.eval_pair_debug(dev(r), dev(w))
        s2 = ctx.eval_pair(dev(r), dev(w))
    jo, h1o, h2o = oc.joint_hist(r, w, shift, bg, bu)
    assert (j == jo).all(), "joint histogram differs"
    assert (h1 == h1o).all() and (h2 == h2o).all(), "marginal histogram differs"
    with oc.rounded():
        so, sums_o = oc.score_from_hist(jo, h1o, h2o, h * wd, mode)
    assert (sums.view(np.uint32) == sums_o.view(np.uint32)).all(), (sums, sums_o)          # bit for bit
    assert np.float32(s).view(np.uint32) == np.float32(so).view(np.uint32) or (np.isnan(s) and np.isnan(so)), (s, so)
    sl, _ = oc.score_from_hist(jo, h1o, h2o, h * wd, mode)                                  # libm log2f cross-check
    assert abs(float(s) - float(sl)) <= SCORE_TOL * max(1.0, abs(float(sl))) or (np.isnan(s) and np.isnan(sl)), (s, sl)
    assert s == s2 or (np.isnan(s) and np.isnan(s2))
    return s


@pytest.mark.parametrize("shape", [(640, 480), (960, 540), (848, 480), (64, 48), (333, 251), (1, 1), (4096, 4096)])
def test_term_table_equals_oracle(nmi, shape):
    """The per-count term table (c/len)*log2(c/len), len = W*H (NMI.cu:242-263): every entry equals the oracle's
    correctly rounded evaluation, and the libm evaluation differs from it by at most one fp32 rounding of the product."""
    from oracle import binding as oc
    w, h = shape
    with nmi.NmiContext(w, h) as ctx:
        got = ctx.term_table()
    with oc.rounded():
        exp = oc.term_table(w * h)
    assert got.shape == exp.shape and (got.view(np.uint32) == exp.view(np.uint32)).all()
    libm = oc.term_table(w * h)
    assert np.abs(libm - exp).max() <= 6e-8 and got[0] == 0 and got[-1] == 0


def test_golden_pairs_all_switches(nmi, golden_pairs, split_mode):
    from oracle import binding as oc
    g = golden_pairs
    for name in g["names"]:
        r, w = g[f"{name}/render"], g[f"{name}/warped"]
        for bg in (1, 0):
            for bu in (1, 0):
                tag = f"{name}/bg{bg}_bu{bu}"
                with nmi.NmiContext(64, 48, use_bg=bool(bg), render_bottom_up=bool(bu)) as ctx:
                    s, j, h1, h2, sums = ctx.eval_pair_debug(dev(r), dev(w))
                assert (j == dense_joint(g, tag)).all(), tag
                assert (h1 == g[f"{tag}/hist_render"]).all() and (h2 == g[f"{tag}/hist_warped"]).all(), tag
                assert (sums == g[f"{tag}/sums_rounded"]).all(), tag
                assert s == g[f"{tag}/score_mode1_rounded"], tag
                assert np.abs(sums - g[f"{tag}/sums"]).max() <= SUM_TOL * max(1, np.abs(g[f"{tag}/sums"]).max()), tag
                assert abs(float(s) - float(g[f"{tag}/score_mode1"])) <= SCORE_TOL, tag
                with nmi.NmiContext(64, 48, mode=nmi.MODE_ENMI, use_bg=bool(bg), render_bottom_up=bool(bu)) as ctx:
                    e = ctx.eval_pair(dev(r), dev(w))
                ref = float(g[f"{tag}/score_mode0"])
                assert (np.isnan(ref) and np.isnan(e)) or abs(float(e) - ref) <= SCORE_TOL * max(1, abs(ref)), tag
                refr = g[f"{tag}/score_mode0_rounded"]
                assert (np.isnan(refr) and np.isnan(e)) or e == refr, tag
                with nmi.NmiContext(64, 48, bins=64, use_bg=bool(bg), render_bottom_up=bool(bu)) as ctx:
                    s64 = ctx.eval_pair(dev(r), dev(w))
                assert abs(float(s64) - float(g[f"{tag}/score64_bins64"])) <= SCORE_TOL, tag
                assert s64 == g[f"{tag}/score64_bins64_rounded"], tag


def test_known_answers_640x480(nmi, golden_kat, split_mode):
    from orbslam2_nmi_amd import synthetic as sy
    a, b = sy.uniform_pair(640, 480, 1234)
    with nmi.NmiContext(640, 480, render_bottom_up=False) as ctx:
        assert abs(float(ctx.eval_pair(dev(a), dev(b))) - 0.0200299) <= 2e-7
        assert ctx.eval_pair(dev(a), dev(a)) == np.float32(1.0)                          # identical
        c, z = np.full_like(a, 255), np.zeros_like(a)
        assert ctx.eval_pair(dev(c), dev(z)) == 0.0                                      # both constant (wrap path)
        assert ctx.eval_pair(dev(c), dev(a)) == 0.0 and ctx.eval_pair(dev(a), dev(c)) == 0.0
    with nmi.NmiContext(640, 480, mode=nmi.MODE_ENMI, render_bottom_up=False) as ctx:
        assert abs(float(ctx.eval_pair(dev(a), dev(b))) - 1.0101162) <= 2e-6
        assert ctx.eval_pair(dev(a), dev(a)) == np.float32(2.0)
    with nmi.NmiContext(640, 480) as ctx:
        assert abs(float(ctx.eval_pair(dev(a), dev(b))) - float(golden_kat["uniform_640x480_seed1234_suc_bottomup"])) <= 2e-7
        assert ctx.eval_pair(dev(a), dev(b)) == golden_kat["uniform_640x480_seed1234_suc_bottomup_rounded"]


@pytest.mark.parametrize("shape", [(640, 480), (960, 540), (848, 480), (64, 48), (16, 4)])
@pytest.mark.parametrize("kind", ["smooth", "uniform"])
def test_pair_vs_oracle_sizes(nmi, shape, kind, split_mode):
    from oracle import binding as oc
    from orbslam2_nmi_amd import synthetic as sy
    w, h = shape
    if kind == "smooth":
        B = sy.scene(w, h, 3)
        r, f = sy.render_stack(B, (1, 1, 1))[0], sy.camera_frame(B, 4)
    else:
        r, f = sy.uniform_pair(w, h, 9)
    for bu in (True, False):
        check_pair(nmi, oc, r, f, bu=bu)
    check_pair(nmi, oc, r, f, bg=False)
    check_pair(nmi, oc, r, f, mode=0)


@pytest.mark.parametrize("shape", [(37, 23), (641, 7), (100, 100), (17, 1), (1, 1), (333, 251)])
def test_ragged_widths_take_the_generic_path(nmi, shape, split_mode):
    from oracle import binding as oc
    w, h = shape
    rng = np.random.default_rng(w * 1000 + h)
    r = rng.integers(0, 256, (h, w), dtype=np.uint8)
    f = np.clip(r.astype(int) + rng.integers(-9, 9, (h, w)), 0, 255).astype(np.uint8)
    for bu in (True, False):
        for bg in (True, False):
            check_pair(nmi, oc, r, f, bg=bg, bu=bu)


@pytest.mark.parametrize("kernel", [0, -1], ids=["grid-kernel", "auto"])
@pytest.mark.parametrize("shape", [(641, 48), (1241, 24), (100, 60), (333, 21), (47, 33), (640, 30)])
def test_grids_whose_rows_are_not_whole_chunks(nmi, shape, kernel):
    """Widths that are not multiples of 16 (KITTI: 1241) and stacks that are not 16-byte aligned: nmi_grid_kernel<GridRows, ..> (floor(W / 16)
    unaligned 16-byte chunks per row + the rows' last pixels one by one), and in automatic mode nmi_pix_kernel, which has the same
    form (such frames never take the row-split kernel: it would read them byte by byte) -- every switch, against the oracle with ==."""
    from oracle import binding as oc
    w, h = shape
    rng = np.random.default_rng(w * 7 + h)
    S, Wn = 5, 4
    base = rng.integers(0, 256, (h, w), dtype=np.uint8)
    rs = np.stack([np.clip(np.roll(base, s - 2, axis=1).astype(int) + rng.integers(-6, 7, (h, w)), 0, 255).astype(np.uint8) for s in range(S)])
    ws = np.stack([np.clip(np.roll(base, v - 1, axis=0).astype(int) + rng.integers(-9, 10, (h, w)), 0, 255).astype(np.uint8) for v in range(Wn)])
    rs[:, :3, :] = 255          # a flat band: folded chunks on this path too
    ws[:, :3, :] = 0
    rs[4] = 200                 # constant pair: one bin takes every pixel (wraps 16 bits when W * H > 65535 -- not at these sizes -- and
    ws[3] = 17                  # takes the flat-region side counters in any case)
    # misaligned copies: the same bytes one byte further on
    buf_r = torch.zeros(rs.size + 16, dtype=torch.uint8, device="cuda")
    buf_w = torch.zeros(ws.size + 16, dtype=torch.uint8, device="cuda")
    for off in ((0, 0), (1, 3)) if w % 16 == 0 else ((0, 0),):
        dr = buf_r[off[0]:off[0] + rs.size].view(S, h, w)
        dw = buf_w[off[1]:off[1] + ws.size].view(Wn, h, w)
        dr.copy_(torch.from_numpy(rs).cuda())
        dw.copy_(torch.from_numpy(ws).cuda())
        for bg, bins, mode, bu in [(True, 256, 1, True), (False, 256, 1, False), (True, 64, 0, True), (False, 32, 1, True), (True, 256, 0, False)]:
            with oc.rounded():
                ro, io, bo = oc.search_grid(rs, ws, render_bottom_up=bu, threads=8, use_bg=bg, mode=mode, shift={256: 0, 64: 2, 32: 3}[bins])
            with nmi.NmiContext(w, h, render_bottom_up=bu, use_bg=bg, mode=mode, bins=bins) as ctx:
                ctx.set_option(ctx.OPT_SPLIT, kernel)  # 0: the one-workgroup-per-candidate kernel, whatever the grid's size
                t = torch.zeros((Wn, S), device="cuda")
                got = ctx.search_grid(dr, dw, t)
                if kernel == -1 and w >= 32 and (bg or bins == 256) and (w % 16 or off != (0, 0)) and ctx.info()["compute_units"] >= 100:
                    assert ctx.pix_status()["last_launch_ranges"] == 5
                pair = ctx.eval_pair(dr[1], dw[2])
                assert pair == ro[2, 1] or (np.isnan(pair) and np.isnan(ro[2, 1]))
            assert got == (io, bo), (shape, off, bg, bins, mode, bu)
            assert (t.cpu().numpy().view(np.uint32) == ro.view(np.uint32)).all(), (shape, off, bg, bins, mode, bu)


def test_rows_form_at_kitti_size_with_counter_wraps(nmi):
    """1241 x 376: a textured pair and a two-level pair whose bins exceed 65,535 hits (optimistic pass fails its pixel-count test,
    the exact pass with returning atomics follows) -- both through the unaligned-row form."""
    from oracle import binding as oc
    w, h = 1241, 376
    rng = np.random.default_rng(5)
    yy, xx = np.mgrid[0:h, 0:w]
    a = rng.integers(0, 256, (h, w), dtype=np.uint8)
    b = np.clip(a.astype(int) + rng.integers(-12, 13, (h, w)), 0, 255).astype(np.uint8)
    two = np.where((xx + yy) % 2 == 0, 10, 200).astype(np.uint8)
    tw2 = np.where((xx // 2 + yy) % 2 == 0, 30, 90).astype(np.uint8)
    rs, ws = np.stack([a, two]), np.stack([b, tw2])
    with oc.rounded():
        ro, io, bo = oc.search_grid(rs, ws, render_bottom_up=True, threads=4)
    with nmi.NmiContext(w, h) as ctx:
        ctx.set_option(ctx.OPT_SPLIT, 0)
        t = torch.zeros((2, 2), device="cuda")
        got = ctx.search_grid(dev(rs), dev(ws), t)
    assert got == (io, bo)
    assert (t.cpu().numpy().view(np.uint32) == ro.view(np.uint32)).all()


@pytest.mark.parametrize("bins", [256, 128, 64, 32, 16])
def test_bins(nmi, bins, split_mode):
    from oracle import binding as oc
    from orbslam2_nmi_amd import synthetic as sy
    B = sy.scene(320, 240, 12)
    check_pair(nmi, oc, sy.render_stack(B, (1, 1, 1))[0], sy.camera_frame(B, 13), bins=bins)
    check_pair(nmi, oc, B, sy.camera_frame(B, 13), bins=bins, bg=False, bu=False)


def test_counter_wrap_cases(nmi, split_mode):
    """Bins above 65535 hits: the packed 16-bit LDS counters wrap and must be reconstructed exactly."""
    from oracle import binding as oc
    w, h = 960, 540  # 518400 pixels: up to 7 wraps of one counter
    rng = np.random.default_rng(77)
    cases = []
    # one bin takes everything, low field / high field / both fields of one LDS word
    cases.append((np.full((h, w), 255, np.uint8), np.zeros((h, w), np.uint8)))
    cases.append((np.full((h, w), 3, np.uint8), np.full((h, w), 200, np.uint8)))
    halves = np.where(np.arange(w)[None, :].repeat(h, 0) < w // 2, 5, 133).astype(np.uint8)  # d2 = 5 and 5+128: same word
    cases.append((np.full((h, w), 9, np.uint8), halves))
    # exactly 65535 / 65536 / 65537 hits in a bin, rest random
    for n in (65535, 65536, 65537, 131071, 131072):
        r = rng.integers(1, 255, h * w).astype(np.uint8)
        f = rng.integers(1, 255, h * w).astype(np.uint8)
        r[:n], f[:n] = 0, 255
        p = rng.permutation(h * w)
        cases.append((r[p].reshape(h, w), f[p].reshape(h, w)))
    # background render (255) over a mostly-black frame plus texture
    r = rng.integers(0, 256, (h, w), dtype=np.uint8)
    r[rng.random((h, w)) < 0.8] = 255
    f = rng.integers(0, 256, (h, w), dtype=np.uint8)
    f[rng.random((h, w)) < 0.7] = 0
    cases.append((r, f))
    for r, f in cases:
        check_pair(nmi, oc, r, f, bu=False)
        check_pair(nmi, oc, r, f, bg=False, bu=True)


def _banded(h, w, values, band):
    """Image of horizontal bands of `band` rows with the given constant values (cycled)."""
    rows = np.array([values[(y // band) % len(values)] for y in range(h)], np.uint8)
    return np.repeat(rows[:, None], w, axis=1)


def test_flat_regions_are_folded_exactly(nmi, split_mode):
    """Regions where both images are constant are folded into weighted adds / 32-bit side counters (fold_flat_chunk):
    few pairs, more distinct pairs than side counters, flat next to texture, flat bins that also collect textured hits
    and exceed 65535, every switch that changes the pixel rule."""
    from oracle import binding as oc
    from orbslam2_nmi_amd import synthetic as sy
    w, h = 640, 480
    rng = np.random.default_rng(5)
    B = sy.scene(w, h, 41)
    tex_r, tex_f = sy.render_stack(B, (1, 1, 1))[0], sy.camera_frame(B, 42)
    cases = []
    # sky: 30 % of the rows flat in both images, the rest textured
    r, f = tex_r.copy(), tex_f.copy()
    r[:144], f[:144] = 255, 255
    cases.append((r, f))
    # 20 bands of 24 rows, 20 distinct (render, frame) pairs: more than the 8 side counters
    cases.append((_banded(h, w, list(range(10, 210, 10)), 24), _banded(h, w, list(range(250, 50, -10)), 24)))
    # bands of 2 rows (1280 px): wavefront-wide agreement only sometimes, lane-level folds mostly
    cases.append((_banded(h, w, [255, 0, 77], 2), _banded(h, w, [0, 255, 200, 130], 2)))
    # vertical stripes 16 px wide: every lane flat, neighbours differ (no wavefront-wide pair)
    stripes = np.repeat((np.arange(w // 16) % 7 * 30).astype(np.uint8), 16)[None, :].repeat(h, 0)
    cases.append((stripes, stripes[:, ::-1].copy()))
    # flat region whose bin also receives scattered textured hits; total above 65535 (high and low field)
    for val in (200, 3):
        r = rng.integers(0, 256, (h, w), dtype=np.uint8)
        f = rng.integers(0, 256, (h, w), dtype=np.uint8)
        r[100:330], f[100:330] = 255, val           # 147200 flat hits
        m = rng.random((h, w)) < 0.05
        r[m], f[m] = 255, val
        cases.append((r, f))
    # zeros: skipped pixels when the background rule is off
    r, f = tex_r.copy(), tex_f.copy()
    r[200:], f[300:] = 0, 0
    cases.append((r, f))
    for r, f in cases:
        check_pair(nmi, oc, r, f, bu=False)
        check_pair(nmi, oc, r, f, bg=False, bu=True)
        check_pair(nmi, oc, r, f, bins=32, bu=True)


def test_flat_regions_in_a_grid(nmi, split_mode2):
    """The grid kernel on stacks with large flat regions: rating table and winner equal the oracle's, with folding on
    and off (NMI_OPT_PHASE_MASK bit 2), so the two code paths are compared with each other too."""
    from oracle import binding as oc
    from orbslam2_nmi_amd import synthetic as sy
    w, h, S, Wn = 320, 240, 6, 5
    wl = sy.workload(w, h, S, Wn, seed=9)
    rs, ws = wl["render_stack"].copy(), wl["warp_stack"].copy()
    rs[:, : h // 3] = 255          # bottom-up renders: these rows meet the frame's last third
    ws[:, -(h // 3):] = 255
    ws[2, : h // 2] = 0
    rs[3, h // 2:] = 255           # render 3 over warp 2: flat (255, 0) as well
    with oc.rounded():
        ref = np.array([[oc.eval_pair(rs[s], ws[v]) for s in range(S)] for v in range(Wn)], np.float32)
    ibest, vbest = oc.find_max(ref)
    with nmi.NmiContext(w, h) as ctx:
        for variant in (3, 0, 1, 4):       # every wrap-handling variant meets the flat regions, with and without folding
            try:
                ctx.set_option(ctx.OPT_HIST_VARIANT, variant)
            except nmi.NmiError as e:      # 0 / 2 / 4 exist only in -DNMI_BUILD_ABLATIONS builds
                assert e.code == -2 and variant in (0, 4)
                continue
            for mask in ((3,) if variant == 4 else (3, 7)):  # bit 2 is a different ablation switch in the pipelined kernel
                ctx.set_option(ctx.OPT_PHASE_MASK, mask)
                ratings = torch.full((Wn, S), -3.0, dtype=torch.float32, device="cuda")
                idx, val = ctx.search_grid(dev(rs), dev(ws), ratings=ratings)
                got = ratings.cpu().numpy()
                assert (got == ref).all(), (variant, mask)
                assert (idx, val) == (ibest, vbest), (variant, mask)


def test_grid_golden(nmi, golden_grid, split_mode):
    g = golden_grid
    rs, ws = g["render_stack"], g["warp_stack"]
    with nmi.NmiContext(64, 48) as ctx:
        ratings = torch.zeros(ws.shape[0], rs.shape[0], dtype=torch.float32, device="cuda")
        idx, best = ctx.search_grid(dev(rs), dev(ws), ratings)
        idx2, best2 = ctx.search_grid(dev(rs), dev(ws))  # without a rating table
    assert idx == int(g["best_index"]) == idx2
    assert abs(float(best) - float(g["best_score"])) <= SCORE_TOL and best == best2
    assert np.abs(ratings.cpu().numpy() - g["ratings"]).max() <= SCORE_TOL
    assert (ratings.cpu().numpy() == g["ratings_rounded"]).all()
    assert idx == int(g["best_index_rounded"]) and best == g["best_score_rounded"]


def grid_vs_oracle(nmi, wl, w, h, **kw):
    from oracle import binding as oc
    rs, ws = wl["render_stack"], wl["warp_stack"]
    S, Wn = rs.shape[0], ws.shape[0]
    with nmi.NmiContext(w, h, render_bottom_up=wl["bottom_up"], **kw) as ctx:
        ratings = torch.full((Wn, S), -7.0, dtype=torch.float32, device="cuda")
        idx, best = ctx.search_grid(dev(rs), dev(ws), ratings)
    with oc.rounded():
        ro, io, bo = oc.search_grid(rs, ws, render_bottom_up=wl["bottom_up"], threads=16,
                                    use_bg=kw.get("use_bg", True), mode=kw.get("mode", 1))
    r = ratings.cpu().numpy()
    assert (r.view(np.uint32) == ro.view(np.uint32)).all(), np.abs(r - ro).max()   # the whole table, bit for bit
    assert (idx, best) == (io, bo)
    assert best == r.reshape(-1)[idx]
    gi, gb = oc.find_max(r)  # arg-max rule applied to the GPU's own table
    assert (gi, gb) == (idx, best)
    return idx, best, r


def test_grid_config2_729_candidates(nmi):
    """BASELINE.json config 2: 640x480, 27 renders x 27 warps, 256 bins; planted optimum at the centre cell."""
    from orbslam2_nmi_amd import synthetic as sy
    wl = sy.workload(640, 480, 27, 27)
    idx, best, _ = grid_vs_oracle(nmi, wl, 640, 480)
    assert idx == wl["planted"] == 364


def test_grid_config3_shape_4096_candidates(nmi):
    """BASELINE.json config 3: 960x540 (ZU-MAV half resolution), 64 renders x 64 warps = 4096 candidates."""
    from orbslam2_nmi_amd import synthetic as sy
    wl = sy.workload(960, 540, 64, 64, seed=77)
    idx, best, r = grid_vs_oracle(nmi, wl, 960, 540)
    assert idx == wl["planted"]
    assert r.shape == (64, 64)


def test_grid_config4_shard_shape(nmi):
    """BASELINE.json config 4, one rank's share: 848x480 (Newer College), 64 of 512 renders x 64 warps, global indices."""
    from oracle import binding as oc
    from orbslam2_nmi_amd import synthetic as sy
    wl = sy.workload(848, 480, 64, 64, seed=5)
    rs, ws = wl["render_stack"], wl["warp_stack"]
    rank, s_total = 3, 512
    with nmi.NmiContext(848, 480) as ctx:
        t = torch.zeros(64, 64, device="cuda")
        key = ctx.search_grid_shard(dev(rs), 64 * rank, s_total, dev(ws), t)
    with oc.rounded():
        ro, io, bo = oc.search_grid(rs, ws, threads=16)
    assert (t.cpu().numpy() == ro).all()
    w, s = divmod(io, 64)
    assert nmi.key_unpack(key) == (w * s_total + 64 * rank + s, bo)


def test_grid_config4_whole_grid_and_its_eight_shards(nmi):
    """BASELINE.json configs[3] at full size on one GPU: 848x480, 512 renders x 64 warps = 32,768 candidates.  The whole rating
    table == the oracle's; then the grid as the 8 ranks of that config would score it (64 renders each, global indices): every
    shard's table is its slice, and the MAX of the 8 packed keys is the whole grid's winner (what the RCCL all-reduce computes)."""
    from oracle import binding as oc
    from orbslam2_nmi_amd import sharding, synthetic as sy
    wl = sy.workload(848, 480, 512, 64, seed=21)
    rs, ws = wl["render_stack"], wl["warp_stack"]
    with oc.rounded():
        ro, io, bo = oc.search_grid(rs, ws, threads=16)
    d_rs, d_ws = dev(rs), dev(ws)
    with nmi.NmiContext(848, 480) as ctx:
        t = torch.zeros(64, 512, device="cuda")
        assert ctx.search_grid(d_rs, d_ws, t) == (io, bo)
        assert (t.cpu().numpy().view(np.uint32) == ro.view(np.uint32)).all()
        assert io == wl["planted"]
        keys = []
        for rank in range(8):
            so, sc, wo, wc = sharding.grid_shard(512, 64, rank, 8)
            assert (so, sc, wo, wc) == (64 * rank, 64, 0, 64)
            ts = torch.zeros(64, 64, device="cuda")
            keys.append(ctx.search_grid_shard(d_rs[so:so + sc], so, 512, d_ws, ts))
            assert (ts.cpu().numpy().view(np.uint32) == ro[:, so:so + sc].view(np.uint32)).all(), rank
        assert nmi.key_unpack(max(keys)) == (io, bo)


def test_full_size_properties_without_oracle(nmi, split_mode):
    """Size-independent properties at full size (no oracle): permutation invariance of the histogram under a common
    pixel permutation, symmetry of SUC in its two images, identical pair -> 1, and arg-max consistency."""
    rng = np.random.default_rng(123)
    w, h = 960, 540
    a = rng.integers(0, 256, (h, w), dtype=np.uint8)
    b = np.clip(a.astype(int) + rng.integers(-30, 30, (h, w)), 0, 255).astype(np.uint8)
    perm = rng.permutation(h * w)
    with nmi.NmiContext(w, h, render_bottom_up=False) as ctx:
        s_ab, j_ab, h1, h2, _ = ctx.eval_pair_debug(dev(a), dev(b))
        s_ba, j_ba, _, _, _ = ctx.eval_pair_debug(dev(b), dev(a))
        s_pp, j_pp, _, _, _ = ctx.eval_pair_debug(dev(a.reshape(-1)[perm].reshape(h, w)), dev(b.reshape(-1)[perm].reshape(h, w)))
        assert (j_ab == j_ba.T).all() and (j_ab == j_pp).all()
        assert j_ab.sum() == h * w and (j_ab.sum(1) == h1).all() and (j_ab.sum(0) == h2).all()
        assert (h1 == np.bincount(a.reshape(-1), minlength=256)).all()
        assert s_pp == s_ab and abs(float(s_ab) - float(s_ba)) <= 1e-6
        assert ctx.eval_pair(dev(b), dev(b)) == np.float32(1.0)
        # a grid whose table is known by construction: renders = {b, a, b}, warps = {a, b}
        rs = torch.stack([dev(b), dev(a), dev(b)])
        ws = torch.stack([dev(a), dev(b)])
        t = torch.zeros(2, 3, device="cuda")
        idx, best = ctx.search_grid(rs, ws, t)
        tt = t.cpu().numpy()
        assert best == np.float32(1.0) and idx == 0 * 3 + 1            # (w=0:a, s=1:a) is the first identical pair
        assert tt[0, 1] == 1.0 and tt[1, 0] == 1.0 and tt[1, 2] == 1.0 and tt[0, 0] == s_ba and tt[1, 1] == s_ab


def test_grid_switches_and_ties(nmi, split_mode):
    from orbslam2_nmi_amd import synthetic as sy
    wl = sy.workload(160, 120, 8, 12, seed=5, bottom_up=False)
    grid_vs_oracle(nmi, wl, 160, 120, use_bg=False)
    grid_vs_oracle(nmi, wl, 160, 120, mode=0)
    # deliberate ties: duplicate the best render and the best warp -> the lowest linear index must win
    rs, ws = wl["render_stack"].copy(), wl["warp_stack"].copy()
    S = rs.shape[0]
    w_c, s_c = divmod(wl["planted"], S)
    rs[1] = rs[s_c]
    rs[6] = rs[s_c]
    ws[0] = ws[w_c]
    ws[11] = ws[w_c]
    wl2 = dict(wl, render_stack=rs, warp_stack=ws)
    idx, best, r = grid_vs_oracle(nmi, wl2, 160, 120)
    assert idx == 0 * S + 1
    assert (r.reshape(-1) == best).sum() == 9


def test_grid_degenerate_tables(nmi, split_mode):
    # every candidate scores 0 (constant renders): winner = first cell with value 0 -> index 0
    rs = np.full((3, 48, 64), 255, np.uint8)
    ws = np.random.default_rng(1).integers(0, 256, (2, 48, 64), dtype=np.uint8)
    with nmi.NmiContext(64, 48) as ctx:
        ratings = torch.full((2, 3), -1.0, device="cuda")
        idx, best = ctx.search_grid(dev(rs), dev(ws), ratings)
        assert (idx, best) == (0, np.float32(0)) and (ratings == 0).all()
        # single candidate
        idx, best = ctx.search_grid(dev(rs[:1]), dev(ws[:1]))
        assert idx == 0


def test_shard_keys_compose(nmi, split_mode):
    """Sharding along the render axis: max over per-shard keys == unsharded winner."""
    from orbslam2_nmi_amd import synthetic as sy
    wl = sy.workload(160, 120, 8, 6, seed=9)
    rs, ws = dev(wl["render_stack"]), dev(wl["warp_stack"])
    with nmi.NmiContext(160, 120) as ctx:
        full = torch.zeros(6, 8, device="cuda")
        idx, best = ctx.search_grid(rs, ws, full)
        for parts in (2, 4, 8):
            n = 8 // parts
            keys, tabs = [], []
            for r in range(parts):
                t = torch.zeros(6, n, device="cuda")
                keys.append(ctx.search_grid_shard(rs[r * n:(r + 1) * n].contiguous(), r * n, 8, ws, t))
                tabs.append(t)
            assert nmi.key_unpack(max(keys)) == (idx, best)
            assert torch.equal(torch.cat(tabs, dim=1), full)
        # the warp axis sharded instead (fewer renders than ranks): blocks of warps, global indices through w_offset
        for parts in (2, 3, 6):
            n = 6 // parts
            keys, tabs = [], []
            for r in range(parts):
                t = torch.zeros(n, 8, device="cuda")
                keys.append(ctx.search_grid_shard(rs, 0, 8, ws[r * n:(r + 1) * n].contiguous(), t, w_offset=r * n, wn_total=6))
                tabs.append(t)
            assert nmi.key_unpack(max(keys)) == (idx, best)
            assert torch.equal(torch.cat(tabs, dim=0), full)
        with pytest.raises(nmi.NmiError):
            ctx.search_grid_shard(rs, 0, 8, ws, w_offset=3, wn_total=6)  # block sticks out of the grid


def test_reuse_of_one_context_is_clean(nmi, split_mode):
    """The LDS histogram is re-zeroed while it is decoded; repeated and interleaved calls must not leak counts."""
    from oracle import binding as oc
    rng = np.random.default_rng(3)
    with nmi.NmiContext(64, 48) as ctx:
        for _ in range(5):
            r = rng.integers(0, 256, (48, 64), dtype=np.uint8)
            f = rng.integers(0, 256, (48, 64), dtype=np.uint8)
            with oc.rounded():
                assert ctx.eval_pair(dev(r), dev(f)) == oc.eval_pair(r, f)
        rs = rng.integers(0, 256, (40, 48, 64), dtype=np.uint8)
        ws = rng.integers(0, 256, (30, 48, 64), dtype=np.uint8)  # 1200 candidates > one pass of workgroups
        t = torch.zeros(30, 40, device="cuda")
        ctx.search_grid(dev(rs), dev(ws), t)
        with oc.rounded():
            ro, _, _ = oc.search_grid(rs, ws, threads=16)
        assert (t.cpu().numpy() == ro).all()


def test_rccl_world_size_1(nmi):
    """The native RCCL entry on one rank (multi-rank runs are the driver's; here: the code path works)."""
    from orbslam2_nmi_amd import capi, synthetic as sy
    wl = sy.workload(64, 48, 4, 3, seed=11)
    rs, ws = dev(wl["render_stack"]), dev(wl["warp_stack"])
    with nmi.NmiContext(64, 48) as ctx:
        ref = ctx.search_grid(rs, ws)
        comm = ctx.rccl_comm_init(capi.rccl_unique_id(), 0, 1)
        try:
            assert ctx.search_grid_rccl(rs, 0, 4, ws, comm) == ref
        finally:
            capi.rccl_comm_destroy(comm)


def test_rccl_empty_shards_do_not_leak_a_stale_winner(nmi):
    """A rank whose block is empty (fewer renders than ranks) still takes part in the all-reduce.  The reduced winner
    must never land in one of the context's ping-pong key slots: the next search on that rank starts its arg-max from
    zero.  Sequence: empty / non-empty calls interleaved, a lower-scoring grid after a higher-scoring one, the
    warp-axis block form; every non-empty result must equal the plain search of the same block."""
    from orbslam2_nmi_amd import capi, synthetic as sy
    rng = np.random.default_rng(8)
    hi_r = rng.integers(0, 256, (4, 48, 64), dtype=np.uint8)
    hi_w = rng.integers(0, 256, (3, 48, 64), dtype=np.uint8)
    hi_w[1] = hi_r[2][::-1]                                       # identical after the bottom-up flip: score 1 at w=1, s=2
    lo_r = rng.integers(0, 256, (4, 48, 64), dtype=np.uint8)      # unrelated noise: every score below 1
    lo_w = rng.integers(0, 256, (3, 48, 64), dtype=np.uint8)
    rs_hi, ws_hi, rs_lo, ws_lo = dev(hi_r), dev(hi_w), dev(lo_r), dev(lo_w)
    empty = torch.zeros((0, 48, 64), dtype=torch.uint8, device="cuda")
    with nmi.NmiContext(64, 48) as ctx:
        ref_hi, ref_lo = ctx.search_grid(rs_hi, ws_hi), ctx.search_grid(rs_lo, ws_lo)
        assert ref_hi == (1 * 4 + 2, np.float32(1.0)) and 0 < ref_lo[1] < 0.9
        comm = ctx.rccl_comm_init(capi.rccl_unique_id(), 0, 1)
        try:
            for _ in range(2):
                assert ctx.search_grid_rccl(rs_hi, 0, 4, ws_hi, comm) == ref_hi
                assert ctx.search_grid_rccl(empty, 0, 4, ws_hi, comm) == (-1, np.float32(0))   # this rank holds no renders
                assert ctx.search_grid_rccl(rs_lo, 0, 4, ws_lo, comm) == ref_lo                  # not hi's stale key
                assert ctx.search_grid_rccl(empty, 4, 4, ws_hi, comm) == (-1, np.float32(0))
                assert ctx.search_grid_rccl(empty, 0, 0, ws_hi, comm) == (-1, np.float32(0))
                assert ctx.search_grid(rs_lo, ws_lo) == ref_lo                                    # and the plain entry too
            # warp-axis block (S < ranks): warps [1, 3) of 3 with global indices
            blk = ctx.search_grid_rccl(rs_hi, 0, 4, ws_hi[1:3].contiguous(), comm, w_offset=1, wn_total=3)
            key = ctx.search_grid_shard(rs_hi, 0, 4, ws_hi[1:3].contiguous(), w_offset=1, wn_total=3)
            assert blk == nmi.key_unpack(key)
            assert ctx.search_grid_rccl(rs_hi, 0, 4, ws_hi[:0].contiguous(), comm, w_offset=0, wn_total=3) == (-1, np.float32(0))
            assert ctx.search_grid_rccl(rs_lo, 0, 4, ws_lo, comm) == ref_lo
        finally:
            capi.rccl_comm_destroy(comm)


def test_alternating_grid_shapes(nmi):
    """A coarse-to-fine search alternates between grid shapes (translation level S x 1, rotation level 1 x Wn, full
    levels): the per-shape visiting orders are cached (more shapes than cache entries here, so entries are evicted
    too) and results must not depend on the order of calls.  Checked against the same context with tiling off."""
    rng = np.random.default_rng(31)
    rs = dev(rng.integers(0, 256, (24, 48, 64), dtype=np.uint8))
    ws = dev(np.clip(rs.cpu().numpy().astype(int) + rng.integers(-40, 40, (24, 48, 64)), 0, 255).astype(np.uint8))
    shapes = [(24, 24), (24, 13), (13, 24), (20, 20), (17, 19), (19, 17), (24, 12), (12, 24), (16, 18), (18, 16), (23, 23), (22, 21),
              (21, 22), (15, 20), (20, 15), (14, 22), (22, 14), (24, 11), (11, 24), (13, 23), (27 // 1 - 3, 1), (1, 24), (3, 9)]
    with nmi.NmiContext(64, 48) as ref_ctx:
        ref_ctx.set_option(ref_ctx.OPT_XCD_TILING, 0)
        ref_ctx.set_option(ref_ctx.OPT_SPLIT, 0)
        expect = {sh: ref_ctx.search_grid(rs[:sh[0]].contiguous(), ws[:sh[1]].contiguous()) for sh in shapes}
    with nmi.NmiContext(64, 48) as ctx:
        for rep in range(3):
            for sh in (shapes if rep != 1 else shapes[::-1]):
                t = torch.zeros(sh[1], sh[0], device="cuda")
                got = ctx.search_grid(rs[:sh[0]].contiguous(), ws[:sh[1]].contiguous(), t)
                assert got == expect[sh], (rep, sh)
                assert t.reshape(-1)[got[0]].item() == got[1]


def test_wait_modes_and_result_paths_agree(nmi):
    """NMI_OPT_WAIT_MODE (spin / yield) and NMI_OPT_RESULT_PATH (mailbox / copy) only change how the host waits."""
    from orbslam2_nmi_amd import synthetic as sy
    wl = sy.workload(160, 120, 9, 9, seed=4)
    rs, ws = dev(wl["render_stack"]), dev(wl["warp_stack"])
    with nmi.NmiContext(160, 120) as ctx:
        ref = ctx.search_grid(rs, ws)
        pair = ctx.eval_pair(rs[0], ws[0])
        for wait in (0, 1):
            for path in (1, 0):
                ctx.set_option(ctx.OPT_WAIT_MODE, wait)
                ctx.set_option(ctx.OPT_RESULT_PATH, path)
                for _ in range(3):
                    assert ctx.search_grid(rs, ws) == ref
                    assert ctx.eval_pair(rs[0], ws[0]) == pair
        assert ctx.info()["workgroups_per_launch"] == ctx.info()["compute_units"]
        ctx.set_option(ctx.OPT_WORKGROUPS, 40)
        assert ctx.info()["workgroups_per_launch"] == 40 and ctx.search_grid(rs, ws) == ref


def test_eval_pairs_equals_single_calls(nmi):
    """nmi_eval_pairs (the batch form behind CUDAF::BeginBatch / Flush): arbitrary (render, warp) pairs, repeated
    pointers, more pairs than one launch holds, an unaligned image (generic pixel path) -- every score equals the
    single-pair call's, bit for bit, and the oracle's."""
    from oracle import binding as oc
    rng = np.random.default_rng(17)
    w, h = 160, 120
    imgs = rng.integers(0, 256, (12, h, w), dtype=np.uint8)
    imgs[3] = np.clip(imgs[0].astype(int) + rng.integers(-20, 20, (h, w)), 0, 255)
    imgs[7][: h // 2] = 255
    d = dev(imgs)
    with nmi.NmiContext(w, h) as ctx:
        assert ctx.eval_pairs([], []).shape == (0,)
        single = {(r, v): ctx.eval_pair(d[r], d[v]) for r in range(12) for v in range(12)}
        for n in (1, 2, 9, 27, 40, 144, 300):
            pairs = [(int(rng.integers(12)), int(rng.integers(12))) for _ in range(n)]
            if n == 27:
                pairs = [(5, v % 12) for v in range(27)]       # one render against many warps: the reference's inner loop
            got = ctx.eval_pairs([d[r] for r, _ in pairs], [d[v] for _, v in pairs])
            assert [np.float32(x) for x in got] == [single[p] for p in pairs], n
        with oc.rounded():
            assert ctx.eval_pairs([d[0]], [d[3]])[0] == oc.eval_pair(imgs[0], imgs[3])
        # an image that does not start on a 16-byte boundary: the batch falls back to the byte-wise pixel loop
        flat = torch.zeros(h * w + 16, dtype=torch.uint8, device="cuda")
        odd = flat[3:3 + h * w].view(h, w)
        odd.copy_(d[4])
        got = ctx.eval_pairs([odd, d[1]], [d[2], odd])
        assert (np.float32(got[0]), np.float32(got[1])) == (single[(4, 2)], single[(1, 4)])
        for mode in (8, 4, 2, 0):   # forced part counts, and the split forms switched off (one pair per launch)
            ctx.set_option(ctx.OPT_SPLIT, mode)
            got = ctx.eval_pairs([d[r] for r in range(12)], [d[(r * 5) % 12] for r in range(12)])
            assert [np.float32(x) for x in got] == [single[(r, (r * 5) % 12)] for r in range(12)], mode


def test_split_hand_off_timeout_falls_back(nmi):
    """The split kernel's scoring workgroup waits (bounded: 2 ms) for the other parts' granules.  If they never come -- here
    one part is told to withhold them; in the field: a neighbour holding compute units -- the kernel posts its epoch to the
    error ring instead of hanging, and the host redoes THAT search with the one-workgroup-per-candidate kernel, pauses the
    split forms for 16 small-grid launches (32, 64 ... when the retry times out again) and then uses them again.  Results stay
    the oracle's throughout."""
    from oracle import binding as oc
    from orbslam2_nmi_amd import synthetic as sy
    wl = sy.workload(160, 120, 3, 2, seed=6)
    rs, ws = dev(wl["render_stack"]), dev(wl["warp_stack"])
    with oc.rounded():
        ro, io, bo = oc.search_grid(wl["render_stack"], wl["warp_stack"])
    with nmi.NmiContext(160, 120) as ctx:
        assert ctx.search_grid(rs, ws) == (io, bo)                      # split kernel (6 candidates -> 8 x 4 parts)
        assert ctx.split_status() == {"timeouts": 0, "cooldown_calls_left": 0, "next_cooldown": 16, "last_launch_parts": 8}
        ctx.set_option(ctx.OPT_PHASE_MASK, 3 | 512)
        t = torch.zeros(2, 3, device="cuda")
        t0 = time.perf_counter()
        assert ctx.search_grid(rs, ws, t) == (io, bo)                   # times out, redone without the split
        assert time.perf_counter() - t0 < 0.025                         # the guard is 2 ms, not 30
        assert (t.cpu().numpy() == ro).all()
        assert "timed out" in ctx._lib.nmi_last_error_detail(ctx._h).decode()
        st = ctx.split_status()
        assert (st["timeouts"], st["cooldown_calls_left"], st["next_cooldown"], st["last_launch_parts"]) == (1, 15, 32, 0)
        assert ctx.eval_pair(rs[1], ws[1]) == ro[1, 1]                  # paused: no second timeout although the switch is still on
        assert ctx.split_status()["timeouts"] == 1 and ctx.split_status()["cooldown_calls_left"] == 14
        ctx.set_option(ctx.OPT_PHASE_MASK, 3)
        for _ in range(14):
            assert ctx.search_grid(rs, ws) == (io, bo)
            assert ctx.split_status()["last_launch_parts"] == 0
        assert ctx.search_grid(rs, ws) == (io, bo)                      # re-armed: the split form is in use again ...
        st = ctx.split_status()
        assert (st["timeouts"], st["cooldown_calls_left"], st["next_cooldown"], st["last_launch_parts"]) == (1, 0, 16, 8)
        ctx.set_option(ctx.OPT_PHASE_MASK, 3 | 512)                     # ... and a retry that fails again doubles the pause
        assert ctx.search_grid(rs, ws) == (io, bo)
        assert ctx.split_status()["cooldown_calls_left"] == 15
        ctx.set_option(ctx.OPT_PHASE_MASK, 3)
        for _ in range(15):
            assert ctx.search_grid(rs, ws) == (io, bo)
        ctx.set_option(ctx.OPT_PHASE_MASK, 3 | 512)
        assert ctx.search_grid(rs, ws) == (io, bo)                      # the retry after the pause times out again: the pause doubles
        st = ctx.split_status()
        assert (st["timeouts"], st["cooldown_calls_left"], st["next_cooldown"]) == (3, 31, 64)
        # an enqueue-only call (nobody would look for a timeout) never uses the split kernel
        ctx.set_option(ctx.OPT_PHASE_MASK, 3)
        for _ in range(32):
            ctx.search_grid(rs, ws)
        st = ctx.split_status()
        assert (st["cooldown_calls_left"], st["next_cooldown"], st["last_launch_parts"]) == (0, 16, 8)
        key = torch.zeros(1, dtype=torch.int64, device="cuda")
        ctx.search_grid_shard(rs, 0, 3, ws, key_out=key, blocking=False)
        assert ctx.split_status()["last_launch_parts"] == 0
        ctx.synchronize()
        assert nmi.key_unpack(int(key.item())) == (io, bo)
    with nmi.NmiContext(160, 120) as ctx:                                # the same for the per-candidate entry
        ctx.set_option(ctx.OPT_PHASE_MASK, 3 | 512)
        assert ctx.eval_pair(rs[2], ws[0]) == ro[0, 2]
        assert ctx.eval_pairs([rs[0], rs[1]], [ws[1], ws[0]]).tolist() == [ro[1, 0], ro[0, 1]]   # paused: pair by pair
        ctx.set_option(ctx.OPT_PHASE_MASK, 3)
        for _ in range(16):
            ctx.eval_pair(rs[2], ws[0])
        ctx.set_option(ctx.OPT_PHASE_MASK, 3 | 512)
        assert ctx.eval_pairs([rs[0], rs[1]], [ws[1], ws[0]]).tolist() == [ro[1, 0], ro[0, 1]]   # batch times out, redone
        assert ctx.split_status()["timeouts"] == 2
    with nmi.NmiContext(160, 120) as ctx:                                # no split form fits: decided before launching
        ctx.set_option(ctx.OPT_WORKGROUPS, 4)
        assert ctx.eval_pairs([rs[0], rs[1]], [ws[1], ws[0]]).tolist() == [ro[1, 0], ro[0, 1]]
        assert ctx.split_status()["last_launch_parts"] == 0


def test_stream_ticket_answers_for_its_own_split_timeout(nmi):
    """Depth-2 stream, two small-grid tickets in flight, the SECOND one's split launch times out: wait(first)
    returns the first's good result, wait(second) notices ITS timeout, redoes the search and returns the oracle's winner and
    table; a ticket whose warp stack has been replaced meanwhile fails with NOT_READY and withholds its table."""
    from oracle import binding as oc
    from orbslam2_nmi_amd import capi, synthetic as sy
    w, h, counts = 160, 120, (3, 1, 1)
    K = sy.intrinsics(w, h)
    B = sy.scene(w, h, 41)
    F = sy.camera_frame(B, 42)
    rs = [sy.render_stack(B, (2, 1, 1), shift_px=2 + i) for i in range(3)]
    Ms = capi.warp_homographies(K, counts, (0.02, 0.02, 0.05))
    with nmi.NmiContext(w, h, render_bottom_up=False) as ctx:
        ws = ctx.warp_stack(dev(F), Ms)
        wsh = ws.cpu().numpy()
        with oc.rounded():
            exp = [oc.search_grid(r, wsh, render_bottom_up=False) for r in rs]
        hf = torch.from_numpy(F).pin_memory()
        hr = [torch.from_numpy(r).pin_memory() for r in rs]
        with nmi.NmiStream(ctx, 2, 3, depth=2) as st:
            st.keep_ratings()
            a = st.submit(hr[0], hf, Ms)
            ctx.set_option(ctx.OPT_PHASE_MASK, 3 | 512)
            b = st.submit(hr[1])
            ctx.set_option(ctx.OPT_PHASE_MASK, 3)
            assert ctx.split_status()["last_launch_parts"] == 8
            assert st.wait(a) == exp[0][1:] and (st.ratings(a, 3, 2) == exp[0][0]).all()
            assert ctx.split_status()["timeouts"] == 0                  # a's check did not consume b's flag
            assert st.wait(b) == exp[1][1:] and (st.ratings(b, 3, 2) == exp[1][0]).all()
            assert ctx.split_status()["timeouts"] == 1
            # first of two times out, the second is an ordinary launch (paused split): each still gets its own answer
            for _ in range(16):
                ctx.search_grid(dev(rs[0]), ws)
            ctx.set_option(ctx.OPT_PHASE_MASK, 3 | 512)
            a = st.submit(hr[2])
            ctx.set_option(ctx.OPT_PHASE_MASK, 3)
            b = st.submit(hr[0])
            assert st.wait(a) == exp[2][1:] and st.wait(b) == exp[0][1:]
            assert ctx.split_status()["timeouts"] == 2
            # a timed-out ticket whose warp stack was refilled by a later frame cannot be redone: NOT_READY, table withheld
            for _ in range(32):
                ctx.search_grid(dev(rs[0]), ws)
            ctx.set_option(ctx.OPT_PHASE_MASK, 3 | 512)
            a = st.submit(hr[1], hf, Ms)
            ctx.set_option(ctx.OPT_PHASE_MASK, 3)
            b = st.submit(hr[2], hf, Ms)
            st.wait(a)                                                  # redone: buffer 1 - a's - is intact (b filled buffer 0)
            st.wait(b)
            for _ in range(64):
                ctx.search_grid(dev(rs[0]), ws)
        with nmi.NmiStream(ctx, 2, 3, depth=3) as st:
            st.keep_ratings()
            ctx.set_option(ctx.OPT_PHASE_MASK, 3 | 512)
            a = st.submit(hr[1], hf, Ms)                                # buffer 0
            ctx.set_option(ctx.OPT_PHASE_MASK, 3)
            b = st.submit(hr[2], hf, Ms)                                # buffer 1
            c = st.submit(hr[0], hf, Ms)                                # buffer 0 again: a's warp stack is gone
            with pytest.raises(nmi.NmiError) as e:
                st.wait(a)
            assert e.value.code == capi.ERR_NOT_READY
            with pytest.raises(nmi.NmiError):
                st.ratings(a, 3, 2)
            assert st.wait(b) == exp[2][1:] and st.wait(c) == exp[0][1:]
            a = st.submit(hr[1])                                        # "submit the level again"
            assert st.wait(a) == exp[1][1:]


def test_split_timeouts_sixteen_launches_apart_are_both_seen(nmi):
    """the ring of per-launch timeout words had 16 entries indexed by epoch & 15 while a stream holds up to 64
    tickets -- a timeout in launch e + 16 overwrote launch e's word, and ticket e returned the key of a timed-out search as
    valid.  18 tickets in flight, the 1st and the 17th time out: both are noticed, redone, and answer with the oracle's winner."""
    from oracle import binding as oc
    from orbslam2_nmi_amd import capi, synthetic as sy
    w, h, counts = 160, 120, (3, 1, 1)
    K = sy.intrinsics(w, h)
    B = sy.scene(w, h, 51)
    F = sy.camera_frame(B, 52)
    rs = [sy.render_stack(B, (2, 1, 1), shift_px=1 + i) for i in range(3)]
    Ms = capi.warp_homographies(K, counts, (0.02, 0.02, 0.05))
    with nmi.NmiContext(w, h, render_bottom_up=False) as ctx:
        ws = ctx.warp_stack(dev(F), Ms)
        wsh = ws.cpu().numpy()
        with oc.rounded():
            exp = [oc.search_grid(r, wsh, render_bottom_up=False) for r in rs]
        hf = torch.from_numpy(F).pin_memory()
        hr = [torch.from_numpy(r).pin_memory() for r in rs]
        with nmi.NmiStream(ctx, 2, 3, depth=20) as st:
            tickets = []
            for i in range(18):
                if i in (0, 16):
                    ctx.set_option(ctx.OPT_PHASE_MASK, 3 | 512)
                tickets.append(st.submit(hr[i % 3], hf, Ms) if i == 0 else st.submit(hr[i % 3]))
                ctx.set_option(ctx.OPT_PHASE_MASK, 3)
                assert ctx.split_status()["last_launch_parts"] == 8
            for i, t in enumerate(tickets):
                assert st.wait(t) == exp[i % 3][1:], i
            assert ctx.split_status()["timeouts"] == 2


def test_invalid_arguments_fail_loudly(nmi):
    with nmi.NmiContext(64, 48) as ctx:
        with pytest.raises(TypeError):
            ctx.eval_pair(torch.zeros(48, 64, dtype=torch.uint8), torch.zeros(48, 64, dtype=torch.uint8))  # host tensors
        with pytest.raises(ValueError):
            ctx.eval_pair(torch.zeros(48, 32, dtype=torch.uint8, device="cuda"), torch.zeros(48, 32, dtype=torch.uint8, device="cuda"))
    with pytest.raises(nmi.NmiError):
        nmi.NmiContext(64, 48, bins=100)


def test_streaming_pipeline_matches_sequential(nmi):
    """BASELINE.json config 5 in small: keyframes x levels streamed from pinned host memory through the double-buffered
    pipeline give the same winners as one blocking search per level on resident stacks."""
    from orbslam2_nmi_amd import capi, synthetic as sy
    w, h, S, counts = 160, 120, 8, (2, 2, 2)
    K = sy.intrinsics(w, h)
    levels = []
    for kf in range(4):
        B = sy.scene(w, h, 300 + kf)
        F = sy.camera_frame(B, 400 + kf)
        for lvl in range(3):
            steps = tuple(s / (2 ** lvl) for s in (0.02, 0.02, 0.05))
            rs = sy.render_stack(B, counts, shift_px=max(1, 4 >> lvl))
            levels.append((kf, lvl, F, rs, capi.warp_homographies(K, counts, steps)))
    with nmi.NmiContext(w, h, render_bottom_up=False) as ctx:
        expected = []
        for kf, lvl, F, rs, Ms in levels:
            ws = ctx.warp_stack(dev(F), Ms)
            expected.append(ctx.search_grid(dev(rs), ws))
        with nmi.NmiStream(ctx, S, 8, depth=2) as st:
            got, pending = [], []
            for kf, lvl, F, rs, Ms in levels:
                hr = torch.from_numpy(rs).pin_memory()
                hf = torch.from_numpy(F).pin_memory()
                # a new frame + warp stack at every level here (steps change); level 0 of each keyframe is the frame switch
                pending.append(st.submit(hr, hf, Ms))
                if len(pending) == 2:
                    got.append(st.wait(pending.pop(0)))
            while pending:
                got.append(st.wait(pending.pop(0)))
            # frame re-use: same frame/warps, another render stack
            t1 = st.submit(torch.from_numpy(levels[-1][3]).pin_memory())
            assert st.wait(t1) == expected[-1]
            # depth exceeded without collecting -> refused, not corrupted
            a = st.submit(torch.from_numpy(levels[0][3]).pin_memory())
            b = st.submit(torch.from_numpy(levels[0][3]).pin_memory())
            with pytest.raises(nmi.NmiError):
                st.submit(torch.from_numpy(levels[0][3]).pin_memory())
            st.wait(a), st.wait(b)
    assert got == expected


@pytest.mark.parametrize("variant", [0, 1, 3, 4])
def test_kernel_variants_agree(nmi, variant):
    """Every exact kernel variant (NMI_OPT_HIST_VARIANT) gives the oracle's table, also on data that wraps counters."""
    from oracle import binding as oc
    from orbslam2_nmi_amd import synthetic as sy
    wl = sy.workload(320, 240, 9, 30, seed=3)          # 270 candidates: several per workgroup when capped below
    rs, ws = wl["render_stack"].copy(), wl["warp_stack"].copy()
    rs[4] = 255                                         # a constant render (76,800 px)...
    ws[7] = 0                                           # ...over a constant frame: one bin gets 76,800 > 65,535 hits
    with oc.rounded():
        ro, io, bo = oc.search_grid(rs, ws, threads=16)
    with nmi.NmiContext(320, 240) as ctx:
        try:
            ctx.set_option(ctx.OPT_HIST_VARIANT, variant)
        except nmi.NmiError as e:
            assert e.code == -2 and variant in (0, 4)
            pytest.skip("ablation variants are not compiled into the shipped library (-DNMI_BUILD_ABLATIONS)")
        ctx.set_option(ctx.OPT_WORKGROUPS, 64)
        t = torch.zeros(30, 9, device="cuda")
        idx, best = ctx.search_grid(dev(rs), dev(ws), t)
    assert (t.cpu().numpy() == ro).all()
    assert (idx, best) == (io, bo)


def test_randomised_shapes_and_switches(nmi, split_mode):
    """Seeded sweep over frame shapes, switches and value distributions (includes flat regions, zeros, saturated pixels):
    histograms bit-exact, score within tolerance, for every draw."""
    from oracle import binding as oc
    rng = np.random.default_rng(20260104)
    for it in range(40):
        w = int(rng.choice([16, 32, 48, 64, 80, 17, 33, 100, 129, 256, 320]))
        h = int(rng.integers(1, 96))
        kind = it % 5
        if kind == 0:
            r = rng.integers(0, 256, (h, w), dtype=np.uint8)
            f = rng.integers(0, 256, (h, w), dtype=np.uint8)
        elif kind == 1:  # few levels -> heavy bins
            r = (rng.integers(0, 3, (h, w)) * 127).astype(np.uint8)
            f = (rng.integers(0, 2, (h, w)) * 255).astype(np.uint8)
        elif kind == 2:  # piecewise flat with zero borders
            r = np.full((h, w), 255, np.uint8)
            r[h // 4:, w // 3:] = rng.integers(0, 256, (h - h // 4, w - w // 3), dtype=np.uint8)
            f = np.zeros((h, w), np.uint8)
            f[: max(1, h // 2)] = rng.integers(1, 256, (max(1, h // 2), w), dtype=np.uint8)
        elif kind == 3:  # smooth ramp + noise
            r = ((np.arange(w)[None, :] * 3 + np.arange(h)[:, None] * 2) % 256).astype(np.uint8)
            f = np.clip(r.astype(int) + rng.integers(-4, 5, (h, w)), 0, 255).astype(np.uint8)
        else:
            r = rng.integers(0, 256, (h, w), dtype=np.uint8)
            f = r.copy()
        check_pair(nmi, oc, r, f, bins=int(rng.choice([256, 64])), mode=int(rng.integers(0, 2)),
                   bg=bool(rng.integers(0, 2)), bu=bool(rng.integers(0, 2)))


def test_empty_grids_and_maximum_frame(nmi, split_mode2):
    """Edge sizes: grids with no candidates give "no winner" (index -1, score 0) without touching the inputs; the largest
    frame the library accepts (4096x4096 = 2^24 pixels, counts still exact in fp32) matches the oracle, wraps included."""
    from oracle import binding as oc
    with nmi.NmiContext(64, 48) as ctx:
        rs0 = torch.zeros((0, 48, 64), dtype=torch.uint8, device="cuda")
        ws = torch.zeros((2, 48, 64), dtype=torch.uint8, device="cuda")
        assert ctx.search_grid(rs0, ws) == (-1, np.float32(0))
        assert ctx.search_grid(ws, rs0) == (-1, np.float32(0))
        assert ctx.search_grid_shard(rs0, 0, 0, ws) == 0
        assert ctx.search_grid(ws[:1], ws[:1])[0] == 0          # and the context still works afterwards
    rng = np.random.default_rng(99)
    n = 4096
    r = rng.integers(0, 256, (n, n), dtype=np.uint8)
    f = np.clip(r.astype(np.int16) + rng.integers(-3, 4, (n, n), dtype=np.int16), 0, 255).astype(np.uint8)
    r[: n // 2, : n // 2] = 255                                   # 4.2 M pixels in one bin: 64 wraps of a 16-bit counter
    f[: n // 2, : n // 2] = 0
    with nmi.NmiContext(n, n, render_bottom_up=False) as ctx:
        s, j, h1, h2, sums = ctx.eval_pair_debug(dev(r), dev(f))
    jo, h1o, h2o = oc.joint_hist(r, f, 0, True, False)
    with oc.rounded():
        so, sums_o = oc.score_from_hist(jo, h1o, h2o, n * n)
    assert (j == jo).all() and (h1 == h1o).all() and (h2 == h2o).all()
    assert j[255, 0] >= (n // 2) ** 2 and s == so and (sums == sums_o).all()


def test_fuzz_campaign_against_the_oracle(nmi):
    """tests/fuzz_parity.py, 250 seeded cases: random grid shapes, frame sizes, switches and content mixes (textured,
    noise, posterised, flat bands / blocks, constant) -- whole rating tables and winners against the C oracle."""
    import fuzz_parity
    assert fuzz_parity.run(250, seed=11, verbose=False) == 0.0   # rating tables equal bit for bit, winners identical
    # the same campaign's first cases through the one-workgroup-per-candidate kernel only (the grids above are small
    # enough that the automatic selection scores most of them with the split kernel)
    assert fuzz_parity.run(60, seed=11, verbose=False, options={nmi.NmiContext.OPT_SPLIT: 0}) == 0.0
    # few-levels path first for every case (quantised content among the kinds): it scores what qualifies and hands the
    # rest back to the general kernel on the device
    C = nmi.NmiContext
    assert fuzz_parity.run(120, seed=12, verbose=False, options={C.OPT_SPLIT: 0, C.OPT_CONTENT_PATH: 1}, kinds=7) == 0.0
    # pixel ranges only (nmi_pix_kernel) for every grid they fit: 3 ranges with the owner's share at its default, 5 with equal
    # shares, 2 with a large bias; grids up to 12 x 12 (mid-size ones among them), ragged widths, every content kind
    for ranges, bias, seed in ((3, 49152, 13), (5, 0, 14), (2, 200000, 15)):
        assert fuzz_parity.run(60, seed=seed, verbose=False, kinds=7, max_side=12,
                               options={C.OPT_SPLIT: 1, C.OPT_SPLIT_PIXELS: ranges, C.OPT_PIX_OWNER_BIAS: bias, C.OPT_CONTENT_PATH: 0}) == 0.0


def test_two_contexts_from_two_threads(nmi):
    """One context per host thread (the library keeps no global mutable state besides the lazily resolved RCCL entry
    points): two threads search different grids at the same time, each on its own context and stream, and every result is
    the one the context gives alone."""
    import threading
    from orbslam2_nmi_amd import synthetic as sy
    jobs = []
    for seed, (w, h, S, Wn) in ((21, (320, 240, 9, 8)), (22, (160, 120, 12, 27))):
        wl = sy.workload(w, h, S, Wn, seed=seed)
        rs, ws = dev(wl["render_stack"]), dev(wl["warp_stack"])
        with nmi.NmiContext(w, h) as ctx:
            expect = ctx.search_grid(rs, ws)
        jobs.append((w, h, rs, ws, expect))
    errors = []

    def worker(job):
        w, h, rs, ws, expect = job
        try:
            with nmi.NmiContext(w, h) as ctx:
                for _ in range(150):
                    got = ctx.search_grid(rs, ws)
                    if got != expect:
                        errors.append((got, expect))
                        return
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))

    threads = [threading.Thread(target=worker, args=(j,)) for j in jobs]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors[:3]
