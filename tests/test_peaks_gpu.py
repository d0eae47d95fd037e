"""GPU tests (-m gpu) of the ranked peaks (include/nmi_hip.h, "Ranked peaks"; csrc/nmi_peaks.hip): nmi_rank_peaks and the peaks
node of a captured level against the numpy model of tests/helpers/peaks_np.py, with == on every key.  Frames are 64 x 48
wherever a search runs."""
import ctypes as C

import numpy as np
import pytest

from helpers import peaks_np as pk

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

W, H = 64, 48
NUM27 = (3, 3, 3, 3, 3, 3)


@pytest.fixture(scope="module")
def nmi():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    import orbslam2_nmi_amd as m
    m.load_library()
    return m


@pytest.fixture(scope="module")
def ctx(nmi):
    with nmi.NmiContext(W, H) as c:
        yield c


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def same(got, want, what):
    assert got[1] == want[1] and got[0].tolist() == want[0].tolist(), what


# ---- every shape, content, radius and K --------------------------------------------------------------------------------------
@pytest.mark.parametrize("num", pk.SHAPES, ids=pk.shape_id)
def test_rank_peaks_equals_the_model(ctx, num):
    for content in pk.CONTENTS:
        t = dev(pk.table(num, content))
        for radius in pk.RADII:
            model = pk.ranked(num, content, radius)
            for K in pk.KS:
                same(ctx.rank_peaks(t, num, K, radius), pk.prefix(model, K), (content, radius, K))
            if content in ("negative", "nan"):
                assert model[1] == 0 and not model[0].any()


def raw_call(nmi, ctx, table, num, K, radius, d_keys, h_keys, count):
    from orbslam2_nmi_amd import capi
    arr = lambda v: None if v is None else (C.c_int32 * 6)(*v)
    return capi.load_library().nmi_rank_peaks(ctx._h, None if table is None else table.data_ptr(), arr(num), K, arr(radius),
                                              None if d_keys is None else d_keys.data_ptr(),
                                              None if h_keys is None else h_keys.ctypes.data_as(C.POINTER(C.c_uint64)),
                                              None if count is None else C.byref(count))


def untouched(d_keys, h_keys, count):
    torch.cuda.synchronize()
    return (d_keys.cpu().numpy() == 7).all() and (h_keys == 9).all() and count.value == -5


def test_a_table_above_the_limit_is_unsupported(nmi, ctx):
    from orbslam2_nmi_amd import capi
    t = torch.rand(65537, device="cuda")
    d_keys, h_keys, count = torch.full((64,), 7, dtype=torch.int64, device="cuda"), np.full(64, 9, np.uint64), C.c_int32(-5)
    for num in (pk.TOO_LARGE, (1, 1, 1, 1, 1, 65537), (256, 256, 2, 1, 1, 1), (2 ** 30, 2 ** 30, 2 ** 30, 2 ** 30, 1, 1)):
        assert raw_call(nmi, ctx, t, num, 8, (1,) * 6, d_keys, h_keys, count) == capi.ERR_UNSUPPORTED, num
        assert untouched(d_keys, h_keys, count), num
    with pytest.raises(nmi.NmiError) as e:
        ctx.rank_peaks(t, pk.TOO_LARGE, 8, (1,) * 6)
    assert e.value.code == capi.ERR_UNSUPPORTED


def test_invalid_arguments_are_refused_with_the_outputs_untouched(nmi, ctx):
    from orbslam2_nmi_amd import capi
    t = torch.rand(729, device="cuda")
    d_keys, h_keys, count = torch.full((64,), 7, dtype=torch.int64, device="cuda"), np.full(64, 9, np.uint64), C.c_int32(-5)
    r1, good = (1,) * 6, NUM27
    bad = [("NULL table", None, good, 8, r1, d_keys, h_keys), ("NULL counts", t, None, 8, r1, d_keys, h_keys),
           ("NULL radius", t, good, 8, None, d_keys, h_keys), ("count 0", t, (3, 3, 0, 3, 3, 3), 8, r1, d_keys, h_keys),
           ("count -1", t, (3, 3, 3, 3, 3, -1), 8, r1, d_keys, h_keys), ("K 0", t, good, 0, r1, d_keys, h_keys),
           ("K -1", t, good, -1, r1, d_keys, h_keys), ("K 65", t, good, 65, r1, d_keys, h_keys),
           ("radius -1", t, good, 8, (1, 1, 1, -1, 1, 1), d_keys, h_keys), ("both outputs NULL", t, good, 8, r1, None, None),
           # a refusal of its own comes before the size limit's
           ("count 0 in a large table", t, (65537, 0, 1, 1, 1, 1), 8, r1, d_keys, h_keys)]
    for what, table, num, K, radius, dk, hk in bad:
        assert raw_call(nmi, ctx, table, num, K, radius, dk, hk, count) == capi.ERR_INVALID_ARGUMENT, what
        assert untouched(d_keys, h_keys, count), what
    lib = capi.load_library()
    assert lib.nmi_rank_peaks(None, t.data_ptr(), (C.c_int32 * 6)(*good), 8, (C.c_int32 * 6)(*r1), d_keys.data_ptr(),
                              h_keys.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(count)) == capi.ERR_INVALID_ARGUMENT
    assert untouched(d_keys, h_keys, count)
    # the same arguments, all good: the call works, and only K keys of each output are written
    assert raw_call(nmi, ctx, t, good, 8, r1, d_keys, h_keys, count) == 0
    want = pk.find_peaks(t.cpu().numpy(), good, 8, r1)
    assert h_keys[:8].tolist() == want[0].tolist() and count.value == want[1] and (h_keys[8:] == 9).all()
    got = d_keys.cpu().numpy()
    assert got[:8].view(np.uint64).tolist() == want[0].tolist() and (got[8:] == 7).all()


def test_a_second_call_equals_a_fresh_contexts(nmi, ctx):
    """Nothing of a call survives it: a large table ranked to the end, then another, then a small one, on one context, each equal
    to what a context that never ranked anything gives."""
    big, small = (16, 16, 16, 4, 2, 2), NUM27
    calls = [(big, "random", (1,) * 6, 64), (big, "holes", (1, 0, 2, 0, 1, 3), 64), (small, "random", (1,) * 6, 64),
             (small, "corners", (1,) * 6, 64), (big, "equal", (100,) * 6, 2), (small, "equal", (0,) * 6, 63)]
    with nmi.NmiContext(W, H) as used:
        for num, content, radius, K in calls:
            t = dev(pk.table(num, content))
            got = used.rank_peaks(t, num, K, radius)
            with nmi.NmiContext(W, H) as fresh:
                same(got, fresh.rank_peaks(t, num, K, radius), (num, content))
            same(got, pk.prefix(pk.ranked(num, content, radius), K), (num, content))


@pytest.mark.parametrize("num", [NUM27, (41, 25, 1, 1, 1, 1), (8, 8, 8, 4, 4, 4)], ids=pk.shape_id)
def test_the_enqueue_only_form_equals_the_blocking_form(ctx, num):
    t = dev(pk.table(num, "holes"))
    for K in (1, 17, 64):
        later = torch.full((K,), -1, dtype=torch.int64, device="cuda")
        both = torch.full((K,), -1, dtype=torch.int64, device="cuda")
        assert ctx.rank_peaks(t, num, K, (1,) * 6, keys_out=later, blocking=False) is None
        keys, count = ctx.rank_peaks(t, num, K, (1,) * 6, keys_out=both)
        ctx.synchronize()
        same((keys, count), pk.prefix(pk.ranked(num, "holes", (1,) * 6), K), K)
        assert later.cpu().numpy().view(np.uint64).tolist() == keys.tolist()
        assert both.cpu().numpy().view(np.uint64).tolist() == keys.tolist()


# ---- against a real search ---------------------------------------------------------------------------------------------------
def test_peaks_of_a_real_search(nmi, ctx):
    from orbslam2_nmi_amd import capi, synthetic as sy
    wl = sy.workload(W, H, 27, 27, seed=77)
    with nmi.NmiContext(W, H, render_bottom_up=wl["bottom_up"]) as c:
        ratings = torch.full((27, 27), -3.0, device="cuda")
        best = c.search_grid(dev(wl["render_stack"]), dev(wl["warp_stack"]), ratings)
        table = ratings.cpu().numpy()
        for radius in pk.RADII:
            keys, count = c.rank_peaks(ratings, NUM27, 16, radius)
            same((keys, count), pk.find_peaks(table, NUM27, 16, radius), radius)
            assert count >= 1 and capi.key_unpack(int(keys[0])) == best


# ---- levels --------------------------------------------------------------------------------------------------------------------
def scene(nmi, c, mesh):
    """-> (dx, da, texture or None, frame, params): a 64 x 48 plane as a cloud or a textured mesh, the camera frame a shifted view
    of it, and params(scale) -> (mvps [27,16], homographies [27,3,3]) of a 3^6 search kernel of steps / scale."""
    from orbslam2_nmi_amd import capi, hostapi as Hh, synthetic as sy
    from test_render import plane_cloud, plane_mesh
    Twc = np.eye(4, dtype=np.float32)
    Twc[:3, 1] = [0, -1, 0]
    pos, look, up = Twc[:3, 3], Twc[:3, 3] + Twc[:3, 2], Twc[:3, 1]
    if mesh:
        xyz, attr, rgb, rp = plane_mesh(W, H, nx=12, ny=9)
        tex = nmi.NmiTexture(c, rgb)
        dx, da = dev(xyz), dev(attr)
        fr = c.render_mesh(dx, da, tex, capi.render_mvp(rp, pos, look, up, (0.05, 0, 0))[None])[0]
    else:
        xyz, attr, rp = plane_cloud(W, H, density=2.0)
        tex = None
        dx, da = dev(xyz), dev(attr)
        fr = c.render_points(dx, torch.sqrt(da), capi.render_mvp(rp, pos, look, up, (0.05, 0, 0))[None], 3.0)[0]
    frame = torch.flip(fr, dims=[0]).contiguous()
    cells = [(sx, sy_, sz) for sz in range(3) for sy_ in range(3) for sx in range(3)]
    K = sy.intrinsics(W, H)

    def params(scale):
        g = Hh.SearchKernel.make(list(NUM27), [s / scale for s in (0.2, 0.2, 0.5, 0.02, 0.02, 0.05)])
        mvps = np.stack([capi.render_mvp(rp, pos, look, up, Hh.calculate_translation(Twc, g, *cell)) for cell in cells])
        return mvps, capi.warp_homographies(K, (3, 3, 3), tuple(g.step[3:6]))
    return dx, da, tex, frame, params


def replay_and_check(lv, base, mvps, Ms, K, radius):
    """One replay of the level with peaks and of its twin without: the peaks equal the model on the level's own table, and the
    winner and the table are the twin's, bit for bit.  -> (winner, table)"""
    from orbslam2_nmi_amd import capi
    win = lv.run(mvps, Ms)
    keys, count = lv.copy_peaks()
    table = lv.outputs()[2]
    same((keys, count), pk.find_peaks(table, NUM27, K, radius), "level peaks")
    assert count >= 1 and capi.key_unpack(int(keys[0])) == win
    assert base.run(mvps, Ms) == win
    assert (base.outputs()[2].view(np.uint32) == table.view(np.uint32)).all()
    return win, table


@pytest.mark.parametrize("kind", ["cloud", "masked-cloud", "mesh"])
def test_level_peaks(nmi, kind):
    from orbslam2_nmi_amd import capi
    mesh = kind == "mesh"
    with nmi.NmiContext(W, H) as c:
        dx, da, tex, frame, params = scene(nmi, c, mesh)
        with nmi.NmiLevel(c, dx, da, frame, 27, 27, 3.0, texture=tex) as lv, nmi.NmiLevel(c, dx, da, frame, 27, 27, 3.0, texture=tex) as base:
            if kind == "masked-cloud":
                lv.set_masks(True, None)
                base.set_masks(True, None)
            with pytest.raises(nmi.NmiError) as e:   # peaks are off
                lv.copy_peaks()
            assert e.value.code == capi.ERR_INVALID_ARGUMENT
            lv.set_peaks(8, NUM27, (1,) * 6)
            first = replay_and_check(lv, base, *params(1.0), 8, (1,) * 6)
            if kind != "cloud":
                return
            second = replay_and_check(lv, base, *params(1.7), 8, (1,) * 6)
            assert (first[1].view(np.uint32) != second[1].view(np.uint32)).any()   # (the two replays do differ)
            # a refused call leaves the level as it was: wrong products, a bad radius, a K too many
            for K, num, radius, code in [(8, (3, 3, 3, 3, 3, 1), (1,) * 6, capi.ERR_INVALID_ARGUMENT),
                                         (8, (3, 3, 9, 3, 3, 3), (1,) * 6, capi.ERR_INVALID_ARGUMENT),
                                         (8, NUM27, (1, 1, -1, 1, 1, 1), capi.ERR_INVALID_ARGUMENT),
                                         (65, NUM27, (1,) * 6, capi.ERR_INVALID_ARGUMENT), (8, None, None, capi.ERR_INVALID_ARGUMENT)]:
                with pytest.raises(nmi.NmiError) as e:
                    lv.set_peaks(K, num, radius)
                assert e.value.code == code, (K, num, radius)
                again = replay_and_check(lv, base, *params(1.0), 8, (1,) * 6)
                assert again[0] == first[0] and (again[1].view(np.uint32) == first[1].view(np.uint32)).all()
            # another K and radius on the same level
            lv.set_peaks(64, NUM27, (1, 0, 2, 0, 1, 3))
            replay_and_check(lv, base, *params(1.7), 64, (1, 0, 2, 0, 1, 3))
            # off again: copy_peaks is refused and the replay equals the first
            lv.set_peaks(0)
            with pytest.raises(nmi.NmiError) as e:
                lv.copy_peaks()
            assert e.value.code == capi.ERR_INVALID_ARGUMENT
            mvps, Ms = params(1.0)
            assert lv.run(mvps, Ms) == first[0]
            assert (lv.outputs()[2].view(np.uint32) == first[1].view(np.uint32)).all()
        if tex is not None:
            tex.close()


def test_level_peaks_on_a_block_are_unsupported(nmi):
    """A block of a sharded level: greedy suppression over a block is not that of the whole grid.  The level stays as it was."""
    from orbslam2_nmi_amd import capi
    with nmi.NmiContext(W, H) as c:
        dx, da, tex, frame, params = scene(nmi, c, False)
        mvps, Ms = params(1.0)
        with nmi.NmiLevel(c, dx, da, frame, 9, 27, 3.0, block=(9, 27, 0, 27)) as lv:
            before = lv.run(mvps[9:18], Ms)
            table = lv.outputs()[2].copy()
            for num in ((3, 3, 1, 3, 3, 3), NUM27):
                with pytest.raises(nmi.NmiError) as e:
                    lv.set_peaks(8, num, (1,) * 6)
                assert e.value.code == capi.ERR_UNSUPPORTED
                with pytest.raises(nmi.NmiError):
                    lv.copy_peaks()
            assert lv.run(mvps[9:18], Ms) == before
            assert (lv.outputs()[2].view(np.uint32) == table.view(np.uint32)).all()
