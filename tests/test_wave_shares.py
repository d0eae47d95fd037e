"""GPU tests (-m gpu) of nmi_grid_kernel's pixel shares by wavefront age (histogram_phase with SLABS, csrc/nmi_grid_device.h): the
16-byte chunks of a candidate are cut into 16 contiguous slabs of unequal length, one per wavefront, from a table of cumulative
Q16 shares.  What can go wrong is a chunk that no slab or two slabs cover, a prefetch or a flat-region resume that leaves its slab,
and the second table (a workgroup's later candidates) -- so the sizes here are the ones where slabs are empty, shorter than a
wavefront's 64 lanes, a whole number of 64-chunk steps or one more, and the contents put a count of their own on every bin they
use, flat blocks on the first and last steps of slabs and across their seams, and more than 65,535 hits on one bin of a
workgroup's second candidate.  Expected joint histograms come from np.add.at in this file; scores, rating tables and winners from
the CPU oracle in its rounded term mode, compared with == (tests/test_gpu_parity.py explains the bar).  The slab table is read
from the header, so the placements follow a re-calibration."""
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SHIFT = {256: 0, 64: 2}
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "orbslam2_nmi_amd", "csrc", "nmi_grid_device.h")


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


def slab_cum():
    """The two rows of 17 cumulative Q16 shares, from the header."""
    src = open(HEADER).read()
    body = re.search(r"slab_cum\[2\]\[kWaves \+ 1\] = \{(.*?)\};", src, re.S).group(1)
    rows = [[int(x) for x in r.split(",")] for r in re.findall(r"\{([^{}]*)\}", body)]
    assert len(rows) == 2 and all(len(r) == 17 and r[0] == 0 and r[16] == 65536 and r == sorted(r) for r in rows)
    return rows


def slab_bounds(n, row=0):
    """Chunk indices [b0, b1, ..., b16]: slab v of n chunks is [b[v], b[v + 1]) (histogram_phase)."""
    return [(n * c) >> 16 for c in slab_cum()[row]]


def np_joint(r, w, shift=0, use_bg=True, bottom_up=False):
    """Joint histogram [render, frame] (NMI.cu:79-87: row y of the frame meets row H-1-y of a bottom-up render), by np.add.at."""
    d1, d2 = (r[::-1] if bottom_up else r).reshape(-1).astype(np.intp), w.reshape(-1).astype(np.intp)
    keep = np.ones(d1.shape, bool) if use_bg else (d1 != 0) & (d2 != 0)
    j = np.zeros((256, 256), np.uint32)
    np.add.at(j, (d1[keep] >> shift, d2[keep] >> shift), 1)
    return j


def distinct_count_pair(h, w, seed):
    """A pair whose k-th bin (of a seeded choice of bins, (0, 0) and bins of row 0 and column 0 among them) holds k + 1 pixels,
    the pixels shuffled over the image: no two bins with the same count, so a chunk read in place of another changes the joint
    histogram, and no flat chunk."""
    rng = np.random.default_rng(seed)
    n = h * w
    nb = int(np.ceil((np.sqrt(8.0 * n + 1) - 1) / 2))
    bins = np.concatenate([[0, 5, 5 * 256, 255 * 256 + 255], rng.choice(65536, nb, replace=False)])
    _, first = np.unique(bins, return_index=True)
    bins = bins[np.sort(first)][:nb]
    px = np.repeat(bins, np.arange(1, nb + 1))[:n]
    rng.shuffle(px)
    return (px >> 8).astype(np.uint8).reshape(h, w), (px & 255).astype(np.uint8).reshape(h, w)


def check_pair(nmi, r, w, bins=256, use_bg=True, bottom_up=False):
    """eval_pair_debug of one pair on nmi_grid_kernel (NMI_OPT_SPLIT 0; its rows form when the width is no multiple of 16): joint
    and marginals against np.add.at, sums and score against the oracle.  -> the joint histogram."""
    from oracle import binding as oc
    h, wd = r.shape
    want = np_joint(r, w, SHIFT[bins], use_bg, bottom_up)
    jo, h1o, h2o = oc.joint_hist(r, w, SHIFT[bins], use_bg, bottom_up)
    assert (np.asarray(jo).reshape(256, 256) == want).all()
    with oc.rounded():
        so, sums_o = oc.score_from_hist(jo, h1o, h2o, h * wd)
    with nmi.NmiContext(wd, h, bins=bins, use_bg=use_bg, render_bottom_up=bottom_up) as ctx:
        ctx.set_option(ctx.OPT_SPLIT, 0)
        s, j, h1, h2, sums = ctx.eval_pair_debug(dev(r), dev(w))
    assert (j == want).all(), np.argwhere(j != want)[:8]
    assert (h1 == want.sum(1)).all() and (h2 == want.sum(0)).all()
    assert (bits(sums) == bits(sums_o)).all(), (sums, sums_o)
    assert bits(s) == bits(so), (s, so)
    return j


def check_grid(nmi, rs, ws, options=None, bins=256, use_bg=True, bottom_up=False):
    """One search of a grid on nmi_grid_kernel: rating table and winner against the oracle's."""
    from oracle import binding as oc
    with oc.rounded():
        ro, io, bo = oc.search_grid(rs, ws, shift=SHIFT[bins], use_bg=use_bg, render_bottom_up=bottom_up, threads=16)
    Wn, S = ws.shape[0], rs.shape[0]
    with nmi.NmiContext(rs.shape[2], rs.shape[1], bins=bins, use_bg=use_bg, render_bottom_up=bottom_up) as ctx:
        ctx.set_option(ctx.OPT_SPLIT, 0)
        for k, v in (options or {}).items():
            ctx.set_option(k, v)
        t = torch.full((Wn, S), -3.0, device="cuda")
        got = ctx.search_grid(dev(rs), dev(ws), t)
        st = ctx.pix_status()
    assert st["last_launch_ranges"] == 0, st
    assert (bits(t.cpu().numpy()) == bits(ro)).all(), options
    assert got == (io, bo), options


# ---- sizes ------------------------------------------------------------------------------------------------------------------
def all_partial_size():
    """(h, w) with w = 208 (13 chunks a row) at which, in both rows of the table, every slab is non-empty and ends in a partial
    64-chunk step."""
    for h in range(100, 200):
        n = 13 * h
        if all(0 < (b[v + 1] - b[v]) and (b[v + 1] - b[v]) % 64 for b in (slab_bounds(n, 0), slab_bounds(n, 1)) for v in range(16)):
            return h, 208
    raise AssertionError("no such size")


def test_slabs_cover_every_chunk_once():
    """The table's arithmetic on its own (no device): at every chunk count the 16 slabs are [0, n) cut in order."""
    for row in (0, 1):
        for n in list(range(1, 2100)) + [19200, 29087, 1 << 20, (1 << 27) - 1]:
            b = slab_bounds(n, row)
            assert b[0] == 0 and b[16] == n and b == sorted(b)
    # what the three smallest sizes below are for: empty slabs, slabs of one to three chunks, every slab shorter than a wavefront
    assert min(np.diff(slab_bounds(8))) == 0 and max(np.diff(slab_bounds(32))) <= 4 and max(np.diff(slab_bounds(192))) < 64


SIZES = {"32x4": (4, 32), "32x16": (16, 32), "64x48": (48, 64), "128x128": (128, 128), "80x205": (205, 80), "partial": None, "rows260x256": (256, 260), "640x480": (480, 640)}


@pytest.mark.parametrize("bottom_up", [False, True], ids=["topdown", "bottomup"])
@pytest.mark.parametrize("size", list(SIZES))
def test_every_size(nmi, size, bottom_up):
    """8 chunks (half of the slabs empty), 32 (slabs of 1 to 3 chunks), 192 (every slab shorter than a wavefront), 1,024 and 1,025, every slab with a partial last
    step, the rows unit (16 whole chunks and 4 single pixels per row), and the benchmark's size."""
    h, w = SIZES[size] or all_partial_size()
    r, f = distinct_count_pair(h, w, 11 + h)
    check_pair(nmi, r, f, bottom_up=bottom_up)


@pytest.mark.parametrize("bottom_up", [False, True], ids=["topdown", "bottomup"])
@pytest.mark.parametrize("use_bg", [True, False], ids=["bg", "bgoff"])
@pytest.mark.parametrize("bins", [256, 64])
@pytest.mark.parametrize("size", ["64x48", "80x205", "rows260x256"])
def test_bins_and_background_rule(nmi, size, bins, use_bg, bottom_up):
    h, w = SIZES[size]
    r, f = distinct_count_pair(h, w, 23 + h)
    check_pair(nmi, r, f, bins, use_bg, bottom_up)


# ---- flat blocks on slab steps ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["first_step", "last_step", "straddling"])
def test_flat_blocks_in_slabs(nmi, where):
    """640 x 480 (19,200 chunks; the youngest wavefronts' slabs are some 300 chunks), textured, with four flat blocks of 128 or 192 chunks (constant render over constant frame, a pair of
    values per block): on the first two steps of the slabs of wavefronts 0, 5, 10, 15 (one of each age class), on their last two,
    or 96 chunks either side of the slab's end (for wavefront 15: of its start).  A wavefront whose step is all flat leaves the fast loop for the
    careful one at that step and must go on inside its slab."""
    h, w = 480, 640
    r, f = distinct_count_pair(h, w, 77)
    r, f = r.reshape(-1).copy(), f.reshape(-1).copy()
    b = slab_bounds(h * w // 16)
    assert min(np.diff(b)) >= 192  # every block inside its slab (or its two)
    for i, v in enumerate((0, 5, 10, 15)):
        if where == "first_step":
            c0, c1 = b[v], b[v] + 128
        elif where == "last_step":
            c0, c1 = b[v + 1] - 128, b[v + 1]
        else:
            seam = b[v + 1] if v < 15 else b[v]
            c0, c1 = seam - 96, seam + 96
        r[16 * c0:16 * c1], f[16 * c0:16 * c1] = 40 + 50 * i, 250 - 60 * i
    j = check_pair(nmi, r.reshape(h, w), f.reshape(h, w))
    assert all(j[40 + 50 * i, 250 - 60 * i] >= 2048 for i in range(4))


# ---- a workgroup's later candidates -----------------------------------------------------------------------------------------------
def test_wrap_on_a_workgroups_second_candidate(nmi):
    """2 renders x 3 frames at 320 x 240 on 2 workgroups, three candidates each; one pair has 67,200 pixels on one bin (14 of every
    16-pixel chunk, so no chunk is flat): the optimistic path's total fails on a candidate in the middle of a workgroup's three and the exact path takes over from there."""
    rng = np.random.default_rng(3)
    h, w = 240, 320
    rs = rng.integers(0, 256, (2, h, w), dtype=np.uint8)
    ws = rng.integers(0, 256, (3, h, w), dtype=np.uint8)
    heavy = (np.arange(w) % 16 != 5) & (np.arange(w) % 16 != 12)
    rs[1][:, heavy], ws[1][:, heavy] = 255, 128
    assert np_joint(rs[1], ws[1])[255, 128] > 65535
    N = nmi.NmiContext
    check_grid(nmi, rs, ws, {N.OPT_WORKGROUPS: 2, N.OPT_CONTENT_PATH: 0})
    check_grid(nmi, rs, ws, {N.OPT_WORKGROUPS: 2})


@pytest.mark.parametrize("bottom_up", [False, True], ids=["topdown", "bottomup"])
def test_grid_27x27_of_small_frames(nmi, bottom_up):
    """729 candidates at 64 x 48 on 243 workgroups: three candidates each, so the second row of shares (wavefront 0's discount) and
    both parities of the double-buffered state are used; with and without the content probe's gated form of the kernel."""
    pairs = [distinct_count_pair(48, 64, 500 + k) for k in range(27)]
    rs = np.stack([p[0] for p in pairs])
    ws = np.stack([p[1] for p in pairs[::-1]])
    N = nmi.NmiContext
    check_grid(nmi, rs, ws, {N.OPT_WORKGROUPS: 243, N.OPT_CONTENT_PATH: 0}, bottom_up=bottom_up)
    check_grid(nmi, rs, ws, {N.OPT_WORKGROUPS: 243}, bottom_up=bottom_up)
