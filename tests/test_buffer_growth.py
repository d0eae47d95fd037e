"""GPU test (-m gpu): the context's, a level's and a stream's device buffers grow, are swapped and are released while work that
may still read them is in flight (csrc/nmi_mem.h: the grow rule and the upload ring, under the real runtime).

Growth depends on counts, not on the frame size, so everything runs on 64x48 frames with growing counts.  On ONE context an
enqueue-only call is followed at once by the call that grows a buffer; every result is compared with == against the oracle in
rounded mode, the fp32 warp twin, or the same call on a fresh context.  Leaks are not looked for here (free device memory moves
under other work on a shared machine): tests/test_device_memory.py counts every allocation on the CPU."""
import numpy as np
import pytest

from helpers import masked_np as mnp
from helpers import undistort_np as unp
from oracle import binding as oc
from oracle import warp_oracle_np as wo
from orbslam2_nmi_amd import capi, synthetic as sy
from test_covered_level import CoveredScene
from test_level_settings_walk import Walk
from test_masked_level import Scene, dev, hood_mask, views
from test_stream_masked import packbits, pin, render_masks

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

W, H, N = 64, 48, 17


@pytest.fixture(scope="module")
def nmi():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    import orbslam2_nmi_amd as m
    m.load_library()
    return m


@pytest.fixture(scope="module")
def stacks():
    """17 renders, 17 warps and their whole rating table by the oracle, rounded mode (== the product's bits): made once."""
    wl = sy.workload(W, H, N, N, seed=7)
    with oc.rounded():
        table, _, _ = oc.search_grid(wl["render_stack"], wl["warp_stack"], threads=4)
    return wl["frame"], wl["render_stack"], wl["warp_stack"], table


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def winner(table):
    """(index, score) of a [Wn, S] table the way the search reports it: the highest score, the lowest index among equals."""
    i = int(np.argmax(table.reshape(-1)))
    return i, table.reshape(-1)[i]


def homographies(n, scale=1.0):
    """n forward homographies: rotations about the x axis in steps of 0.01 * scale rad."""
    return capi.warp_homographies(sy.intrinsics(W, H), (n, 1, 1), (0.01 * scale, 0.02, 0.05))


def test_grids_grow_the_search_buffers_under_an_enqueued_search(nmi, stacks):
    """2x2 (blocking: the split kernel's slabs and blocks), 6x6 (pixel-range blocks), 12x12 (the order table), each enqueued
    without a wait first and then searched by the blocking call of the NEXT size, which grows what that size needs."""
    _, rs, ws, table = stacks
    sizes = (2, 6, 12)
    with nmi.NmiContext(W, H) as ctx:
        d_rs, d_ws = dev(rs), dev(ws)
        queued = {n: torch.full((n, n), -1.0, device="cuda") for n in sizes}
        blocked = {n: torch.full((n, n), -1.0, device="cuda") for n in sizes}
        torch.cuda.synchronize()
        wins = {}
        for n, nxt in zip(sizes, sizes[1:] + sizes[:1]):
            ctx.search_grid_shard(d_rs[:n], 0, n, d_ws[:n], ratings=queued[n], blocking=False)
            wins[nxt] = ctx.search_grid(d_rs[:nxt], d_ws[:nxt], blocked[nxt])
        ctx.synchronize()
        for n in sizes:
            want = table[:n, :n]
            assert (bits(queued[n].cpu().numpy()) == bits(want)).all(), f"enqueue-only {n}x{n}"
            assert (bits(blocked[n].cpu().numpy()) == bits(want)).all(), f"blocking {n}x{n}"
            assert wins[n] == winner(want), (n, wins[n], winner(want))


def test_seventeen_grid_shapes_evict_an_order_table_in_use(nmi, stacks):
    """The order cache holds 16 shapes: 17 enqueue-only searches of distinct shapes in a row (small and unchecked: nmi_grid_kernel
    with its visiting order), then the first shape again, which was evicted while its launch may not have started."""
    _, rs, ws, table = stacks
    with nmi.NmiContext(W, H) as ctx:
        d_rs, d_ws = dev(rs), dev(ws)
        shapes = [(s, 1) for s in range(1, N + 1)] + [(1, 1), (2, 3)]
        out = [torch.full((wn, s), -1.0, device="cuda") for s, wn in shapes]
        torch.cuda.synchronize()
        for (s, wn), t in zip(shapes, out):
            ctx.search_grid_shard(d_rs[:s], 0, s, d_ws[:wn], ratings=t, blocking=False)
        ctx.synchronize()
        for (s, wn), t in zip(shapes, out):
            assert (bits(t.cpu().numpy()) == bits(table[:wn, :s])).all(), (s, wn)


def mask_stacks():
    rng = np.random.default_rng(11)
    wm = (rng.random((5, H, W)) > 0.2).astype(np.uint8)
    return wm, render_masks(4, W, H, 12)


def test_masked_and_covered_searches_grow_their_counts_tables_and_redo_list(nmi, stacks):
    """Masked searches of 2, 5, 2 warps and covered searches of 2x2, 4x5, 2x2 on one context, an enqueued plain search before each,
    against the same single call on a fresh context."""
    _, rs, ws, _ = stacks
    wm, rm = mask_stacks()
    calls = [("masked", 3, 2), ("masked", 3, 5), ("covered", 2, 2), ("covered", 4, 5), ("masked", 3, 2), ("covered", 2, 2)]

    def one(ctx, kind, s, wn, d, busy=None):
        t = torch.full((wn, s), -1.0, device="cuda")
        torch.cuda.synchronize()
        if busy is not None:
            ctx.search_grid_shard(d["rs"][:6], 0, 6, d["ws"][:6], ratings=busy, blocking=False)
        if kind == "masked":
            win = ctx.search_grid_masked(d["rs"][:s], d["ws"][:wn], d["wm"][:wn], t)
            cnt = ctx.mask_counts(wn)
        else:
            win = ctx.search_grid_covered(d["rs"][:s], d["rm"][:s], d["ws"][:wn], d["wm"][:wn], t)
            cnt = ctx.cover_counts(wn * s)
        return win, bits(t.cpu().numpy()), cnt

    d = {"rs": dev(rs), "ws": dev(ws), "wm": dev(wm), "rm": dev(rm)}
    with nmi.NmiContext(W, H) as ctx:
        busy = torch.zeros(6, 6, device="cuda")
        got = [one(ctx, kind, s, wn, d, busy) for kind, s, wn in calls]
    for (kind, s, wn), (win, tab, cnt) in zip(calls, got):
        with nmi.NmiContext(W, H) as fresh:
            win2, tab2, cnt2 = one(fresh, kind, s, wn, d)
        assert win == win2 and (tab == tab2).all() and (cnt == cnt2).all(), (kind, s, wn)
        if kind == "masked":
            assert (cnt == np.count_nonzero(wm[:wn].reshape(wn, -1), axis=1)).all()


def test_eval_pairs_grows_its_tables_across_the_256_floor(nmi, stacks):
    _, rs, ws, table = stacks
    with nmi.NmiContext(W, H) as ctx:
        d_rs, d_ws = dev(rs), dev(ws)
        for n in (3, 300, 3, 300):
            si, wi = [(5 * i) % N for i in range(n)], [(3 * i + 1) % N for i in range(n)]
            got = ctx.eval_pairs([d_rs[s] for s in si], [d_ws[w] for w in wi])
            assert (bits(got) == bits(table[wi, si])).all(), n


def test_warp_rings_grow_and_wrap_without_a_wait(nmi, stacks):
    """nmi_warp_stack and nmi_warp_stack_masked with 2, then 9 warps, then six calls back to back with no wait between them (the
    ring has four slots): every stack against the fp32 twin, every mask stack against its model."""
    F = stacks[0]
    fm = hood_mask(W, H)
    runs = [(2, 1.0), (9, 1.0)] + [(9, 0.5 + 0.25 * k) for k in range(6)]
    with nmi.NmiContext(W, H) as ctx:
        d_F, d_fm = dev(F), dev(fm)
        plain = [torch.empty((n, H, W), dtype=torch.uint8, device="cuda") for n, _ in runs]
        masked = [(torch.empty((n, H, W), dtype=torch.uint8, device="cuda"), torch.empty((n, H, W), dtype=torch.uint8, device="cuda")) for n, _ in runs]
        torch.cuda.synchronize()
        for (n, scale), p, (m, mm) in zip(runs, plain, masked):
            ctx.warp_stack(d_F, homographies(n, scale), out=p, sync=False)
            ctx.warp_stack_masked(d_F, homographies(n, scale), d_fm, out=m, out_masks=mm, sync=False)
        ctx.synchronize()
        for (n, scale), p, (m, mm) in zip(runs, plain, masked):
            Ms = homographies(n, scale)
            want = wo.warp_stack(F, Ms)
            assert (p.cpu().numpy() == want).all() and (m.cpu().numpy() == want).all(), (n, scale)
            assert (mm.cpu().numpy() == mnp.warp_masks((H, W), Ms, fm)).all(), (n, scale)


def test_renders_grow_the_view_ring_the_anchors_and_the_mesh_work_area(nmi):
    """Point renders of 1, then 4 views and mesh renders of 1, then 3 views, enqueued without a wait between them, against the
    same single call on a fresh context."""
    def scene(ctx, mesh):
        sc = Scene(nmi, ctx, W, H, mesh)
        return sc, views(sc.rp, 4)

    def render(ctx, sc, mesh, mvps, out):
        if mesh:
            ctx.render_mesh(sc.dx, sc.da, sc.tex, mvps, out=out, sync=False)
        else:
            ctx.render_points(sc.dx, sc.da, mvps, 3.0, out=out, sync=False)

    counts = (1, 4, 1, 3, 4)
    with nmi.NmiContext(W, H) as ctx:
        scenes = {mesh: scene(ctx, mesh) for mesh in (False, True)}
        outs = {(mesh, i): torch.empty((n, H, W), dtype=torch.uint8, device="cuda") for mesh in scenes for i, n in enumerate(counts)}
        torch.cuda.synchronize()
        for i, n in enumerate(counts):
            for mesh, (sc, mvps) in scenes.items():
                render(ctx, sc, mesh, mvps[:n], outs[mesh, i])
        ctx.synchronize()
        got = {k: v.cpu().numpy() for k, v in outs.items()}
        for sc, _ in scenes.values():
            if sc.tex is not None:
                sc.tex.close()
    for mesh in (False, True):
        for i, n in enumerate(counts):
            with nmi.NmiContext(W, H) as fresh:
                sc, mvps = scene(fresh, mesh)
                out = torch.empty((n, H, W), dtype=torch.uint8, device="cuda")
                render(fresh, sc, mesh, mvps[:n], out)
                fresh.synchronize()
                assert (got[mesh, i] == out.cpu().numpy()).all(), (mesh, i, n)
                if sc.tex is not None:
                    sc.tex.close()


@pytest.mark.parametrize("mesh", [False, True], ids=["cloud", "mesh"])
def test_a_level_switched_through_its_settings_and_back(nmi, mesh):
    """Masked, covered, distorted, reduced and back to the level as created: after each switch one run against a fresh level put
    straight into that state (tests/test_level_settings_walk.py's check), so a buffer released too early or kept stale shows."""
    with nmi.NmiContext(W, H) as ctx:
        wk = Walk(nmi, ctx, W, H, mesh, 16, 3, 3)
        path = [("plain", "none", "off"), ("masked", "none", "off"), ("plain", "none", "off"), ("covered", "none", "off"),
                ("covered", "barrel", "off"), ("covered", "barrel", "reduced"), ("plain", "barrel", "reduced"), ("masked", "barrel", "reduced"),
                ("masked", "none", "reduced"), ("masked", "none", "off"), ("plain", "none", "off")]
        with wk.fresh() as lv:
            wk.check(lv, path[0], "as created")
            for src, dst in zip(path[:-1], path[1:]):
                if src[0] != dst[0]:
                    wk.set_kind(lv, src[0], dst[0])
                elif src[1] != dst[1]:
                    wk.set_lens(lv, dst[1])
                else:
                    wk.set_frame(lv, dst[2])
                wk.check(lv, dst, f"{src} -> {dst}")


def test_a_stream_switched_through_its_ticket_kinds_and_back(nmi, stacks):
    """Plain, masked, covered, distorted masked, distorted covered tickets and back to plain on one stream (its mask, coverage
    and undistortion buffers appear on the way), each against a fresh stream that submits that ticket alone."""
    F, rs, _, _ = stacks
    S, Wn = 4, 3
    Ms = homographies(Wn)
    fm = hood_mask(W, H)
    _, rm = mask_stacks()
    K, dist = sy.intrinsics(W, H), unp.FAMILIES["barrel"]
    h_rs, h_F, h_fm, h_bits = pin(rs[:S]), pin(F), pin(fm), pin(packbits(rm))
    steps = [("plain", False), ("masked", False), ("covered", False), ("masked", True), ("covered", True), ("plain", True), ("plain", False),
             ("covered", False)]

    def ticket(st, kind, lens):
        st.set_distortion(K, dist if lens else None)
        if kind == "plain":
            t = st.submit(h_rs, h_F, Ms)
        elif kind == "masked":
            t = st.submit_masked(h_rs, h_F, h_fm, Ms)
        else:
            t = st.submit_covered(h_rs, h_bits, h_F, h_fm, Ms)
        win = st.wait(t)
        cnt = st.counts(t, Wn if kind == "masked" else Wn * S) if kind != "plain" else np.zeros(0, np.int32)
        return win, bits(st.ratings(t, Wn, S)), cnt

    with nmi.NmiContext(W, H) as ctx:
        with nmi.NmiStream(ctx, S, Wn, depth=2) as st:
            st.keep_ratings()
            got = [ticket(st, kind, lens) for kind, lens in steps]
        for (kind, lens), (win, tab, cnt) in zip(steps, got):
            with nmi.NmiStream(ctx, S, Wn, depth=2) as ref:
                ref.keep_ratings()
                win2, tab2, cnt2 = ticket(ref, kind, lens)
            assert win == win2 and (tab == tab2).all() and (cnt == cnt2).all(), (kind, lens)


def test_twenty_rounds_of_create_use_destroy(nmi, stacks):
    """Context, texture, level and stream created, each used once and destroyed -- the children in either order, the context
    last -- twenty times over; every round's results equal the first round's."""
    F, rs, ws, table = stacks
    S, Wn = 3, 3
    Ms = homographies(Wn)
    h_rs, h_F = pin(rs[:S]), pin(F)
    first = None
    for round_ in range(20):
        ctx = nmi.NmiContext(W, H)
        sc = CoveredScene(nmi, ctx, W, H, True)   # (makes the texture and renders the frame: the mesh work area, the view ring)
        lv = sc.level(S, Wn)
        st = nmi.NmiStream(ctx, S, Wn, depth=2)
        t = torch.full((Wn, S), -1.0, device="cuda")
        win = ctx.search_grid(dev(rs[:S]), dev(ws[:Wn]), t)
        assert (bits(t.cpu().numpy()) == bits(table[:Wn, :S])).all() and win == winner(table[:Wn, :S])
        got = (lv.run(views(sc.rp, S), Ms), st.wait(st.submit(h_rs, h_F, Ms)))
        first = first or got
        assert got == first, round_
        for child in ((lv, st) if round_ % 2 else (st, lv)):
            child.close()
        sc.tex.close()
        ctx.close()
