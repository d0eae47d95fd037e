"""GPU tests (-m gpu) of the kept frame marginal in nmi_grid_kernel (csrc/nmi_grid_kernel.h, decode_phase<.., KEPT> and final_phase's
`kept` in csrc/nmi_grid_device.h) and of the visiting order that feeds it (build_search_order, csrc/nmi_search_plan.h): a workgroup
whose candidates stay on one warp forms the frame marginal and its entropy sum on the first of them only.  What can go wrong is a
marginal kept across a change of warp, across a launch, into or out of the exact path after a counter wrap, with the background
rule off, or a warp whose marginal the content probe no longer sees -- so every case here compares the whole rating table and the
winner with the CPU oracle in its rounded term mode, with == (tests/test_gpu_parity.py explains the bar).  Frames are 64 x 48 (192
chunks: the smallest size at which all 16 wavefront slabs get work), 320 x 240 where a bin has to pass 65,535 hits, and 640 x 480
once."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SHIFT = {256: 0, 64: 2}


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


def stacks(S, Wn, h=48, w=64, seed=1):
    """Textured stacks; the warps hold levels below 128 and one pixel of 128 + k in warp k, so no two warps share a marginal."""
    rng = np.random.default_rng(seed)
    rs = rng.integers(0, 256, (S, h, w), dtype=np.uint8)
    ws = rng.integers(0, 128, (Wn, h, w), dtype=np.uint8)
    for k in range(Wn):
        ws[k].reshape(-1)[:128] = np.arange(128)
        ws[k, h // 2, (7 * k) % w] = 128 + k
    return rs, ws


_ORACLE = {}


def oracle(key, rs, ws, bins=256, use_bg=True, bottom_up=False):
    """(ratings, index, best) of the CPU oracle, computed once per key."""
    from oracle import binding as oc
    k = (key, bins, use_bg, bottom_up)
    if k not in _ORACLE:
        with oc.rounded():
            _ORACLE[k] = oc.search_grid(rs, ws, shift=SHIFT[bins], use_bg=use_bg, render_bottom_up=bottom_up, threads=16)
    return _ORACLE[k]


def search(ctx, rs, ws, want):
    ro, io, bo = want
    t = torch.full((ws.shape[0], rs.shape[0]), -3.0, device="cuda")
    got = ctx.search_grid(dev(rs), dev(ws), t)
    assert ctx.pix_status()["last_launch_ranges"] == 0 and ctx.split_status()["last_launch_parts"] == 0  # nmi_grid_kernel's launch
    r = t.cpu().numpy()
    assert (bits(r) == bits(ro)).all(), np.argwhere(bits(r) != bits(ro))[:8]
    assert got == (io, bo)


def check(nmi, key, rs, ws, options=None, bins=256, use_bg=True, bottom_up=False):
    want = oracle(key, rs, ws, bins, use_bg, bottom_up)
    N = nmi.NmiContext
    with N(rs.shape[2], rs.shape[1], bins=bins, use_bg=use_bg, render_bottom_up=bottom_up) as ctx:
        ctx.set_option(N.OPT_SPLIT, 0)
        for k, v in (options or {}).items():
            ctx.set_option(k, v)
        search(ctx, rs, ws, want)
        return ctx.last_content()


@pytest.mark.parametrize("bottom_up", [False, True], ids=["topdown", "bottomup"])
@pytest.mark.parametrize("bins", [256, 64])
@pytest.mark.parametrize("workgroups", [243, 256])
def test_27x27_one_warp_per_workgroup(nmi, workgroups, bins, bottom_up):
    """Three candidates per workgroup on 243, three or two on 256, all on the workgroup's warp; the content probe off (the plain
    kernel, no plan) and on."""
    rs, ws = stacks(27, 27)
    N = nmi.NmiContext
    check(nmi, "27x27", rs, ws, {N.OPT_WORKGROUPS: workgroups, N.OPT_CONTENT_PATH: 0}, bins, bottom_up=bottom_up)
    check(nmi, "27x27", rs, ws, {N.OPT_WORKGROUPS: workgroups}, bins, bottom_up=bottom_up)


@pytest.mark.parametrize("workgroups", [243, 256, 8])
def test_content_probe_sees_every_warp(nmi, workgroups):
    """Renders of 8 levels, warps of the same 8 plus one pixel of a level of their own: the first search of a context runs on
    nmi_grid_kernel as its own probe and posts 8 x 35 levels (a change of verdict, so it is posted) only if the frame marginal of
    every warp was ORed in -- by the candidate that formed it.  (The ORs of a warp's s == 0 candidate are issued in the
    workgroup's first round here, long before the last workgroup's ticket reads the masks.)"""
    rng = np.random.default_rng(6)
    rs = (10 * rng.integers(0, 8, (27, 48, 64))).astype(np.uint8)
    ws = (10 * rng.integers(0, 8, (27, 48, 64))).astype(np.uint8)
    for k in range(27):
        ws[k, 24, (7 * k) % 64] = 128 + k
    info = check(nmi, "fewlevels", rs, ws, {nmi.NmiContext.OPT_WORKGROUPS: workgroups})
    assert (info["nr"], info["nw"]) == (8, 8 + 27), info


@pytest.mark.parametrize("S,Wn,workgroups", [(5, 7, 0), (5, 7, 8), (1, 9, 0), (1, 9, 2), (9, 1, 0), (9, 1, 2), (3, 3, 8), (3, 3, 2), (27, 4, 8)],
                         ids=lambda v: str(v))
def test_partial_or_no_sharing(nmi, S, Wn, workgroups):
    """Shapes whose order stays the tiles (5 x 7; one render; one warp, where a workgroup's run of candidates is on one warp all the
    same), 3 x 3 on 8 workgroups (one workgroup with two candidates of one warp, seven with one) and on 2 (tiles: four or five
    candidates per workgroup, the warp changes mid-way, kept and formed marginals alternate), and 27 x 4 on 8: 13 or 14 candidates
    per workgroup, one warp each."""
    rs, ws = stacks(S, Wn, seed=10 + S)
    N = nmi.NmiContext
    check(nmi, ("small", S, Wn), rs, ws, {N.OPT_WORKGROUPS: workgroups} if workgroups else None)


def test_background_rule_off_forms_every_marginal(nmi):
    """Rule off at 256 bins (the skipped pixels depend on both images: nothing is kept) and at 64 (the exact-only instantiation),
    with zeros in both stacks."""
    rs, ws = stacks(27, 27, seed=5)
    rs[rs < 24] = 0
    ws[ws < 12] = 0
    N = nmi.NmiContext
    for bins in (256, 64):
        check(nmi, "bgoff", rs, ws, {N.OPT_WORKGROUPS: 243}, bins, use_bg=False)


@pytest.mark.parametrize("heavy_render", [0, 1, 2], ids=["first", "middle", "last"])
def test_wrap_meets_the_kept_marginal(nmi, heavy_render):
    """3 renders x 2 warps at 320 x 240 on 2 workgroups: workgroup 0 scores warp 0 against renders 0, 1, 2 in that order.  One of
    the three pairs has 67,200 pixels on one bin (14 of every 16-pixel chunk, so no chunk is flat): the count test fails on the
    workgroup's first, middle or last candidate, and the exact path takes over with a marginal kept before it, or none."""
    rng = np.random.default_rng(3)
    h, w = 240, 320
    rs = rng.integers(0, 256, (3, h, w), dtype=np.uint8)
    ws = rng.integers(0, 256, (2, h, w), dtype=np.uint8)
    heavy = (np.arange(w) % 16 != 5) & (np.arange(w) % 16 != 12)
    rs[heavy_render][:, heavy], ws[0][:, heavy] = 255, 128
    assert int(((rs[heavy_render] == 255) & (ws[0] == 128)).sum()) > 65535
    N = nmi.NmiContext
    for opts in ({N.OPT_WORKGROUPS: 2, N.OPT_CONTENT_PATH: 0}, {N.OPT_WORKGROUPS: 2}):
        check(nmi, ("wrap", heavy_render), rs, ws, opts)


def test_rows_unit(nmi):
    """Width 62: rows of 3 whole chunks and 14 single pixels, nmi_grid_kernel<GridRows, ..>; 9 x 9 on 27 workgroups, three candidates each."""
    rs, ws = stacks(9, 9, h=48, w=62, seed=8)
    N = nmi.NmiContext
    check(nmi, "rows", rs, ws, {N.OPT_WORKGROUPS: 27})
    check(nmi, "rows", rs, ws, {N.OPT_WORKGROUPS: 27}, bins=64)


def test_gated_unit_behind_the_few_levels_kernels(nmi):
    """NMI_OPT_CONTENT_PATH 1 sends the search to the few-levels kernels, whose probe finds 256 x 155 levels and hands it back on
    the device: nmi_grid_kernel<GridGated, ..> scores it, on the tile order (this launch's table is the few-levels kernels')."""
    rs, ws = stacks(27, 27)
    N = nmi.NmiContext
    info = check(nmi, "27x27", rs, ws, {N.OPT_WORKGROUPS: 243, N.OPT_CONTENT_PATH: 1})
    assert not info["few_levels"], info


def test_no_order_table(nmi):
    """NMI_OPT_XCD_TILING 0: candidates in ordinal order, p = w * 27 + s; on 243 workgroups a workgroup's three are 243 apart, nine
    warps apart (nothing kept), on 9 workgroups they are 81 of three warps in runs of 27."""
    rs, ws = stacks(27, 27)
    N = nmi.NmiContext
    check(nmi, "27x27", rs, ws, {N.OPT_WORKGROUPS: 243, N.OPT_XCD_TILING: 0})
    check(nmi, "27x27", rs, ws, {N.OPT_WORKGROUPS: 9, N.OPT_XCD_TILING: 0})


def test_two_warp_stacks_in_turn(nmi):
    """One context, two searches with different warp stacks, then the first again: nothing of a launch survives it."""
    rs, ws1 = stacks(27, 27)
    _, ws2 = stacks(27, 27, seed=2)
    N = nmi.NmiContext
    with N(64, 48, bins=256, use_bg=True, render_bottom_up=False) as ctx:
        ctx.set_option(N.OPT_SPLIT, 0)
        ctx.set_option(N.OPT_WORKGROUPS, 243)
        search(ctx, rs, ws1, oracle("27x27", rs, ws1))
        search(ctx, rs, ws2, oracle("27x27b", rs, ws2))
        search(ctx, rs, ws1, oracle("27x27", rs, ws1))
        ctx.set_option(N.OPT_WORKGROUPS, 256)  # another grid: another order of the same shape
        search(ctx, rs, ws2, oracle("27x27b", rs, ws2))


def test_640x480_once(nmi):
    """The benchmark's search: 27 x 27 at 640 x 480 on one workgroup per compute unit."""
    rs, ws = stacks(27, 27, h=480, w=640, seed=4)
    check(nmi, "vga", rs, ws)
