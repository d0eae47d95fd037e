"""GPU tests (-m gpu) of the packed joint histogram's LDS layout (csrc/nmi_grid_device.h): joint rows 129 words apart, decoded
in passes whose rows are 16 apart.  What can go wrong with a skewed stride is aliasing between neighbouring rows, a count in
one of the unused gap words, and a key (wrap event, flat-region side counter, pixel-range unit) that is turned back into the
wrong row -- so the contents here put counts on every bin once, on the corners of the 128-bin halves, and more than 65,535
hits on bins of the last and the first row.  Expected joint histograms come from np.add.at in this file; scores, rating tables
and winners from the CPU oracle in its rounded term mode, compared with == (tests/test_gpu_parity.py explains the bar)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SHIFT = {256: 0, 64: 2}
CORNERS = np.array([0, 1, 127, 128, 254, 255], np.uint8)


@pytest.fixture(scope="module")
def nmi():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    import orbslam2_nmi_amd as m
    m.load_library()
    return m


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def np_joint(r, w, shift=0, use_bg=True):
    """Joint histogram [render, frame] of a top-down pair (NMI.cu:79-87), by np.add.at."""
    d1, d2 = r.reshape(-1).astype(np.intp), w.reshape(-1).astype(np.intp)
    keep = np.ones(d1.shape, bool) if use_bg else (d1 != 0) & (d2 != 0)
    j = np.zeros((256, 256), np.uint32)
    np.add.at(j, (d1[keep] >> shift, d2[keep] >> shift), 1)
    return j


def routes(nmi):
    """A single pair's default route is the row-split kernel, which has a layout of its own: the pair is also sent to
    nmi_grid_kernel (NMI_OPT_SPLIT 0; its rows form when the width is no multiple of 16) and to the pixel-range kernel with 3
    ranges, whose owner decodes its helpers' units beside its own counters."""
    N = nmi.NmiContext
    return [{N.OPT_SPLIT: 0}, {N.OPT_SPLIT: 1, N.OPT_SPLIT_PIXELS: 3}, {}]


def check_pair(nmi, r, w, bins=256, use_bg=True):
    """eval_pair_debug of one top-down pair on every route: joint and marginals against np.add.at, sums and score against the
    oracle.  -> (joint, marginals) of the nmi_grid_kernel route."""
    from oracle import binding as oc
    h, wd = r.shape
    want = np_joint(r, w, SHIFT[bins], use_bg)
    jo, h1o, h2o = oc.joint_hist(r, w, SHIFT[bins], use_bg, False)
    assert (jo == want).all()
    with oc.rounded():
        so, sums_o = oc.score_from_hist(jo, h1o, h2o, h * wd)
    out = None
    for options in routes(nmi):
        with nmi.NmiContext(wd, h, bins=bins, use_bg=use_bg, render_bottom_up=False) as ctx:
            for k, v in options.items():
                ctx.set_option(k, v)
            s, j, h1, h2, sums = ctx.eval_pair_debug(dev(r), dev(w))
        assert (j == want).all(), (options, np.argwhere(j != want)[:8])
        assert (h1 == want.sum(1)).all() and (h2 == want.sum(0)).all(), options
        assert (bits(sums) == bits(sums_o)).all(), (options, sums, sums_o)
        assert bits(s) == bits(so), (options, s, so)
        out = out or (j, h1, h2)
    return out


def check_grid(nmi, rs, ws, options=None, bins=256, use_bg=True):
    """One search of a top-down grid: rating table and winner against the oracle's.  -> pix_status of the launch."""
    from oracle import binding as oc
    with oc.rounded():
        ro, io, bo = oc.search_grid(rs, ws, shift=SHIFT[bins], use_bg=use_bg, render_bottom_up=False, threads=16)
    Wn, S = ws.shape[0], rs.shape[0]
    with nmi.NmiContext(rs.shape[2], rs.shape[1], bins=bins, use_bg=use_bg, render_bottom_up=False) as ctx:
        for k, v in (options or {}).items():
            ctx.set_option(k, v)
        t = torch.full((Wn, S), -3.0, device="cuda")
        got = ctx.search_grid(dev(rs), dev(ws), t)
        st = ctx.pix_status()
        cus = ctx.info()["compute_units"]
    assert (bits(t.cpu().numpy()) == bits(ro)).all(), options
    assert got == (io, bo), options
    return st, cus


# ---- every bin once ---------------------------------------------------------------------------------------------------------
def every_bin_pairs():
    yy, xx = np.mgrid[0:256, 0:256]
    rng = np.random.default_rng(129)
    p1, p2 = rng.permutation(256), rng.permutation(256)
    return {"rows_by_columns": (yy, xx), "transposed": (xx, yy), "permuted": (p1[yy], p2[xx])}


@pytest.mark.parametrize("which", ["rows_by_columns", "transposed", "permuted"])
def test_every_bin_once(nmi, which):
    """256 x 256 pixels, one on each of the 65,536 bins: any two bins that share a counter, and any count that lands in a gap
    word, shows as a joint histogram that is not all ones."""
    r, w = (a.astype(np.uint8) for a in every_bin_pairs()[which])
    j, h1, h2 = check_pair(nmi, r, w)
    assert (j == 1).all() and (h1 == 256).all() and (h2 == 256).all()


@pytest.mark.parametrize("which", ["rows_by_columns", "transposed", "permuted"])
def test_every_bin_once_through_the_rows_kernel(nmi, which):
    """The same content at a width that is no multiple of 16 (260: unaligned rows and 4 tail pixels per row, the rows kernel);
    the padding pixels sit on bin (0, 0), which then holds 1 + 4 * 256."""
    r0, w0 = (a.astype(np.uint8) for a in every_bin_pairs()[which])
    r, w = np.zeros((256, 260), np.uint8), np.zeros((256, 260), np.uint8)
    r[:, :256], w[:, :256] = r0, w0
    j, h1, h2 = check_pair(nmi, r, w)
    want = np.ones((256, 256), np.uint32)
    want[0, 0] = 1 + 4 * 256
    assert (j == want).all() and h1[0] == 256 + 1024 and h2[0] == 256 + 1024 and (h1[1:] == 256).all() and (h2[1:] == 256).all()


# ---- corners ----------------------------------------------------------------------------------------------------------------
def corner_image_pair(seed, h=48, w=64):
    """Both images over {0, 1, 127, 128, 254, 255}: all 36 combinations present, with unequal seeded weights."""
    rng = np.random.default_rng(seed)
    combo = np.concatenate([np.arange(36), rng.choice(36, h * w - 36, p=rng.dirichlet(np.ones(36)))])
    rng.shuffle(combo)
    return CORNERS[combo // 6].reshape(h, w), CORNERS[combo % 6].reshape(h, w)


@pytest.mark.parametrize("bins", [256, 64])
@pytest.mark.parametrize("use_bg", [True, False], ids=["bg", "bgoff"])
def test_corners(nmi, use_bg, bins):
    """First and last rows, first and last words of a row, both sides of the 128-bin seam of a packed word; background rule
    off is where the decode clears row 0 and column 0."""
    r, w = corner_image_pair(7)
    j, _, _ = check_pair(nmi, r, w, bins, use_bg)
    assert np.count_nonzero(j) == {(256, True): 36, (256, False): 25, (64, True): 16, (64, False): 16}[(bins, use_bg)]


# ---- wraps in the last rows ---------------------------------------------------------------------------------------------------
HEAVY = [(255, 255), (255, 127), (255, 128), (0, 0)]


def heavy_pair(d1, d2, flat, seed):
    """320 x 240 with more than 65,535 pixels on bin (d1, d2).  Textured: 14 of every 16-pixel chunk (67,200 pixels), the two
    others random, so no chunk is flat and the exact path sees 16-bit wraps; flat: the first 207 rows whole (66,240 pixels),
    which the flat-region fold puts on side counters."""
    rng = np.random.default_rng(seed)
    h, w = 240, 320
    r = rng.integers(0, 256, (h, w), dtype=np.uint8)
    f = rng.integers(0, 256, (h, w), dtype=np.uint8)
    if flat:
        r[:207], f[:207] = d1, d2
    else:
        heavy = (np.arange(w) % 16 != 5) & (np.arange(w) % 16 != 12)
        r[:, heavy], f[:, heavy] = d1, d2
    return r, f


@pytest.mark.parametrize("flat", [False, True], ids=["texture", "flat"])
@pytest.mark.parametrize("d1,d2", HEAVY)
def test_wraps_in_the_last_rows(nmi, d1, d2, flat):
    """A 16-bit field that wraps (or a side counter that stands in for it) on the last joint row's last word, on both fields of
    its seam words and on the first word of all: the keys that name these counters are turned back into the right row."""
    r, f = heavy_pair(d1, d2, flat, 1000 + d1 + d2)
    j, _, _ = check_pair(nmi, r, f)
    assert j[d1, d2] > 65535
    # ... and as one cell of a 2 x 2 grid (the default routing, and nmi_grid_kernel itself)
    rng = np.random.default_rng(5)
    rs = np.stack([rng.integers(0, 256, r.shape, dtype=np.uint8), r])
    ws = np.stack([f, rng.integers(0, 256, r.shape, dtype=np.uint8)])
    N = nmi.NmiContext
    check_grid(nmi, rs, ws)
    check_grid(nmi, rs, ws, {N.OPT_SPLIT: 0})


# ---- the pixel-range hand-off in the new decode order ---------------------------------------------------------------------------
def test_grid_9x9_of_corner_content(nmi):
    """81 candidates at 64 x 48: the default routing hands helpers' units to owners in decode order (pixel-range kernel); with
    it switched off nmi_grid_kernel scores the same grid."""
    pairs = [corner_image_pair(100 + k) for k in range(9)]
    rs = np.stack([p[0] for p in pairs])
    ws = np.stack([p[1] for p in pairs])
    N = nmi.NmiContext
    st, cus = check_grid(nmi, rs, ws)
    if cus == 256:
        assert st["last_launch_ranges"] > 1, st
    assert st["healed"] == 0
    st, _ = check_grid(nmi, rs, ws, {N.OPT_SPLIT: 0})
    assert st["last_launch_ranges"] == 0, st
