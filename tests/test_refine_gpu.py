"""GPU tests (-m gpu) of the refined peaks (include/nmi_hip.h, "Refined peaks"; csrc/nmi_refine.hip): nmi_refine_peaks and the
refine node of a captured level against the float32 numpy model of tests/helpers/refine_np.py, with == on every byte of every
record, and against its float64 model on planted quadratics the CPU tier did not see.  Tables only, or 64 x 48 frames where a
level runs."""
import ctypes as C

import numpy as np
import pytest

from helpers import peaks_np as pk
from helpers import refine_np as rf

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

W, H = 64, 48
NUM27 = (3, 3, 3, 3, 3, 3)
f32 = np.float32


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


def dev_keys(keys):
    return dev(np.asarray(keys, np.uint64).view(np.int64))


def same(got, want, what):
    assert rf.same_bytes(got, want), (what, rf.explain(got, want))


# ---- every shape, content, radius and K, keys from the device and from the host ----------------------------------------------
@pytest.mark.parametrize("num", rf.GPU_SHAPES, ids=pk.shape_id)
def test_refine_peaks_equals_the_model(ctx, num):
    for content in rf.CONTENTS:
        t = dev(rf.table(num, content))
        for radius in rf.RADII:
            keys, want = rf.keys_of(num, content, radius), rf.refined(num, content, radius)
            for K in rf.KS:
                same(ctx.refine_peaks(t, num, keys[:K]), want[:K], (content, radius, K, "host keys"))
                same(ctx.refine_peaks(t, num, dev_keys(keys[:K])), want[:K], (content, radius, K, "device keys"))
    if num == NUM27:   # the peak of the bowl is interior on all six axes: all 73 samples
        first = rf.refined(num, "bowl", (1,) * 6)[0]
        assert first["flags"] == rf.COUPLED and first["offset"].all() and first["hessian"].all()


def test_three_qualifying_cells_give_sixty_one_empty_records(ctx):
    num = (5, 13, 1, 1, 1, 1)
    keys = rf.keys_of(num, "few", (0,) * 6)
    assert np.count_nonzero(keys) == 3
    got = ctx.refine_peaks(dev(rf.table(num, "few")), num, keys)
    same(got, rf.refined(num, "few", (0,) * 6), "few")
    assert (got["flags"][3:] == rf.EMPTY).all() and not got["key"][3:].any() and (got["key"][:3] == keys[:3]).all()


def test_a_key_that_names_no_cell_gives_an_empty_record(nmi, ctx):
    """An index at or past the number of cells is an input the rule defines: the record is empty and the table is not read."""
    from orbslam2_nmi_amd import capi
    num = (5, 13, 1, 1, 1, 1)
    t = rf.table(num, "random")
    good = rf.keys_of(num, "random", (1,) * 6)
    keys = np.array([good[0], capi.key_pack(1.0, 65), capi.key_pack(1.0, 2 ** 31), good[1], capi.key_pack(1.0, 2 ** 32 - 2), 0], np.uint64)
    want = rf.refine(t, num, keys, f32)
    assert (want["flags"][[1, 2, 4, 5]] == rf.EMPTY).all() and want["key"][0] == good[0] and want["key"][3] == good[1]
    same(ctx.refine_peaks(dev(t), num, keys), want, "host keys")
    same(ctx.refine_peaks(dev(t), num, dev_keys(keys)), want, "device keys")


def test_a_table_above_the_peaks_limit(nmi, ctx):
    """65,537 cells: nmi_rank_peaks refuses it, this kernel only gathers.  Keys from the host."""
    num = rf.ABOVE_PEAKS_LIMIT
    t = pk.table(num, "holes")
    keys, count = pk.find_peaks(t, num, 16, (1,) * 6)
    assert count == 16
    keys[5] = pk.keys_of(t)[65536] or keys[5]   # the last cell among them, whatever it holds
    same(ctx.refine_peaks(dev(t), num, keys), rf.refine(t, num, keys, f32), num)


# ---- the enqueue-only form -----------------------------------------------------------------------------------------------------
def test_the_enqueue_only_form_runs_in_stream_order_behind_a_search(nmi):
    from orbslam2_nmi_amd import synthetic as sy
    wl = sy.workload(W, H, 27, 27, seed=77)
    with nmi.NmiContext(W, H, render_bottom_up=wl["bottom_up"]) as c:
        ratings = torch.full((27, 27), -3.0, device="cuda")
        d_keys = torch.zeros(8, dtype=torch.int64, device="cuda")
        d_records = torch.full((8 * 152,), 0x5A, dtype=torch.uint8, device="cuda")
        renders, warps = dev(wl["render_stack"]), dev(wl["warp_stack"])
        d_win = torch.zeros(1, dtype=torch.int64, device="cuda")
        assert c.search_grid_shard(renders, 0, 27, warps, ratings, key_out=d_win, blocking=False) is None   # the whole grid, enqueued
        assert c.rank_peaks(ratings, NUM27, 8, (1,) * 6, keys_out=d_keys, blocking=False) is None
        assert c.refine_peaks(ratings, NUM27, d_keys, records_out=d_records, blocking=False) is None
        c.synchronize()
        table = ratings.cpu().numpy()
        keys = pk.find_peaks(table, NUM27, 8, (1,) * 6)[0]
        assert d_keys.cpu().numpy().view(np.uint64).tolist() == keys.tolist() and int(d_win.cpu().numpy().view(np.uint64)[0]) == int(keys[0])
        assert (table != -3.0).all()                  # the search did write it
        want = rf.refine(table, NUM27, keys, f32)
        same(d_records.cpu().numpy().view(rf.record_dtype(f32)), want, "enqueue only")
        # the blocking form with both outputs: the same records in both
        d_records.fill_(0x5A)
        got = c.refine_peaks(ratings, NUM27, d_keys, records_out=d_records)
        same(got, want, "blocking")
        same(d_records.cpu().numpy().view(rf.record_dtype(f32)), want, "blocking, device copy")


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_are_refused_with_the_outputs_untouched(nmi, ctx):
    from orbslam2_nmi_amd import capi
    lib = capi.load_library()
    t = torch.rand(729, device="cuda")
    before = t.clone()
    d_keys = dev_keys(pk.find_peaks(t.cpu().numpy(), NUM27, 8, (1,) * 6)[0])
    h_keys = d_keys.cpu().numpy().view(np.uint64).copy()
    d_out = torch.full((64 * 152,), 7, dtype=torch.uint8, device="cuda")
    h_out = np.full(64 * 152, 9, np.uint8)
    arr = lambda v: None if v is None else (C.c_int32 * 6)(*v)
    hk = h_keys.ctypes.data_as(C.POINTER(C.c_uint64))

    def call(handle, table, num, dk, hkeys, K, do, ho):
        return lib.nmi_refine_peaks(handle, None if table is None else table.data_ptr(), arr(num), None if dk is None else dk.data_ptr(), hkeys, K,
                                    None if do is None else do.data_ptr(), None if ho is None else ho.ctypes.data)

    def untouched():
        torch.cuda.synchronize()
        return bool((d_out == 7).all()) and (h_out == 9).all() and bool((t == before).all())

    bad = [("NULL context", None, t, NUM27, d_keys, None, 8, d_out, h_out), ("NULL table", ctx._h, None, NUM27, d_keys, None, 8, d_out, h_out),
           ("NULL counts", ctx._h, t, None, d_keys, None, 8, d_out, h_out), ("count 0", ctx._h, t, (3, 3, 0, 3, 3, 3), d_keys, None, 8, d_out, h_out),
           ("count -1", ctx._h, t, (3, 3, 3, 3, 3, -1), d_keys, None, 8, d_out, h_out), ("K 0", ctx._h, t, NUM27, d_keys, None, 0, d_out, h_out),
           ("K -1", ctx._h, t, NUM27, None, hk, -1, d_out, h_out), ("K 65", ctx._h, t, NUM27, None, hk, 65, d_out, h_out),
           ("both keys", ctx._h, t, NUM27, d_keys, hk, 8, d_out, h_out), ("no keys", ctx._h, t, NUM27, None, None, 8, d_out, h_out),
           ("no output", ctx._h, t, NUM27, d_keys, None, 8, None, None)]
    for what, handle, table, num, dk, hkeys, K, do, ho in bad:
        assert call(handle, table, num, dk, hkeys, K, do, ho) == capi.ERR_INVALID_ARGUMENT, what
        assert untouched(), what
    # indices that do not fit a key's 32 bits
    assert call(ctx._h, t, (65536, 65536, 1, 1, 1, 1), d_keys, None, 8, d_out, h_out) == capi.ERR_UNSUPPORTED and untouched()
    # the same arguments, all good: the call works, and only K records of each output are written
    want = rf.refine(before.cpu().numpy(), NUM27, h_keys, f32)
    for dk, hkeys in ((d_keys, None), (None, hk)):
        assert call(ctx._h, t, NUM27, dk, hkeys, 8, d_out, h_out) == 0
        assert h_out[:8 * 152].tobytes() == want.tobytes() and (h_out[8 * 152:] == 9).all()
        got = d_out.cpu().numpy()
        assert got[:8 * 152].tobytes() == want.tobytes() and (got[8 * 152:] == 7).all() and bool((t == before).all())
        d_out.fill_(7)
        h_out[:] = 9


# ---- levels --------------------------------------------------------------------------------------------------------------------
def replay_and_check(lv, base, mvps, Ms, K):
    """One replay of the level with refined peaks and of its twin without: the records equal the model on the level's own table
    and keys, and the winner and the table are the twin's, bit for bit."""
    win = lv.run(mvps, Ms)
    keys, count = lv.copy_peaks()
    records, n = lv.copy_refined()
    table = lv.outputs()[2]
    same(records, rf.refine(table, NUM27, keys, f32), "level records")
    assert n == count >= 1 and len(records) == K and records["key"][0] == keys[0]
    assert base.run(mvps, Ms) == win
    assert (base.outputs()[2].view(np.uint32) == table.view(np.uint32)).all()
    return win


@pytest.mark.parametrize("kind", ["cloud", "masked-cloud", "mesh"])
def test_level_refined_peaks(nmi, kind):
    from orbslam2_nmi_amd import capi
    from test_peaks_gpu import scene
    with nmi.NmiContext(W, H) as c:
        dx, da, tex, frame, params = scene(nmi, c, kind == "mesh")
        with nmi.NmiLevel(c, dx, da, frame, 27, 27, 3.0, texture=tex) as lv, nmi.NmiLevel(c, dx, da, frame, 27, 27, 3.0, texture=tex) as base:
            if kind == "masked-cloud":
                lv.set_masks(True, None)
                base.set_masks(True, None)

            def refused(call, code=capi.ERR_INVALID_ARGUMENT):
                with pytest.raises(nmi.NmiError) as e:
                    call()
                assert e.value.code == code

            refused(lv.set_refine)       # peaks are off
            refused(lv.copy_refined)
            lv.set_peaks(4, NUM27, (1,) * 6)
            refused(lv.copy_refined)     # refine is off
            lv.set_refine(True)
            first = replay_and_check(lv, base, *params(1.0), 4)
            if kind != "cloud":
                return
            # a reconfigure: masks on, then off; the records follow the level's table each time
            lv.set_masks(True, None)
            base.set_masks(True, None)
            replay_and_check(lv, base, *params(1.0), 4)
            lv.set_masks(False, None)
            base.set_masks(False, None)
            assert replay_and_check(lv, base, *params(1.0), 4) == first
            # another K while refine is on
            lv.set_peaks(64, NUM27, (0,) * 6)
            replay_and_check(lv, base, *params(1.7), 64)
            # refine off and on again; then the peaks off, which takes refine with them
            lv.set_refine(False)
            refused(lv.copy_refined)
            assert lv.run(*params(1.0)) == first and lv.copy_peaks()[1] == 64
            lv.set_refine(True)
            replay_and_check(lv, base, *params(1.0), 64)
            lv.set_peaks(0)
            refused(lv.copy_refined)
            refused(lv.set_refine)
            assert lv.run(*params(1.0)) == first
            lv.set_peaks(4, NUM27, (1,) * 6)
            refused(lv.copy_refined)     # turning the peaks on again does not bring refine back
        if tex is not None:
            tex.close()


def test_level_refine_on_a_block_is_refused(nmi):
    from orbslam2_nmi_amd import capi
    from test_peaks_gpu import scene
    with nmi.NmiContext(W, H) as c:
        dx, da, tex, frame, params = scene(nmi, c, False)
        mvps, Ms = params(1.0)
        with nmi.NmiLevel(c, dx, da, frame, 9, 27, 3.0, block=(9, 27, 0, 27)) as lv:
            before = lv.run(mvps[9:18], Ms)
            table = lv.outputs()[2].copy()
            with pytest.raises(nmi.NmiError) as e:
                lv.set_refine(True)
            assert e.value.code == capi.ERR_UNSUPPORTED
            with pytest.raises(nmi.NmiError):
                lv.copy_refined()
            assert lv.run(mvps[9:18], Ms) == before
            assert (lv.outputs()[2].view(np.uint32) == table.view(np.uint32)).all()


# ---- accuracy on seeds the CPU tier did not use ----------------------------------------------------------------------------------
@pytest.mark.parametrize("magnitude", sorted(rf.MAGNITUDES))
def test_accuracy_on_unseen_seeds(ctx, magnitude):
    cases = [c for seed in rf.GPU_SEEDS for c in rf.planted(seed, magnitude)]
    kept = worst_offset = worst_score = 0
    for t64, offset, A in cases:
        k = rf.kept(t64)
        if k is None:
            continue
        kept += 1
        t32, m64 = k
        got = ctx.refine_peaks(dev(t32), NUM27, [rf.centre_key(t32)])[0]
        assert got["flags"] == rf.COUPLED
        worst_offset = max(worst_offset, np.abs(got["offset"].astype(np.float64) - m64["offset"]).max())
        worst_score = max(worst_score, abs(float(got["score"]) - m64["score"]))
    print(f"{magnitude}: kept {kept} of {len(cases)}, device against float64: offset {worst_offset:.3g} cells, score {worst_score:.3g}")
    assert kept >= 0.9 * len(cases)
    assert worst_offset <= rf.OFFSET_TOLERANCE and worst_score <= rf.SCORE_TOLERANCE
