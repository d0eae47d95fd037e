"""Distorted keyframe streams on the GPU (-m gpu): nmi_stream_set_distortion (include/nmi_hip.h).

Plain, masked and covered tickets (and their _block forms without a communicator) on raw frames equal the standalone chain
nmi_undistort_frame -> nmi_warp_stack[_masked] -> nmi_search_grid[_masked / _covered]: winner, score bits, rating tables,
counts.  A frame-less ticket in between reuses the latest warps; tickets submitted before the setting changes keep theirs; and
zero coefficients give the tickets of a stream that never had distortion."""
import numpy as np
import pytest

from helpers import undistort_np as unp
from orbslam2_nmi_amd import synthetic as sy
from test_stream_masked import hood, level, pin, render_masks

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

LENS = unp.FAMILIES["pincushion"]


@pytest.fixture(scope="module")
def nmi():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    import orbslam2_nmi_amd as m
    m.load_library()
    return m


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def standalone(ctx, kind, K, dist, F, fm, rs, rm, Ms):
    """-> (winner, ratings, counts or None) of the chain on the raw frame F (dist None: no undistortion)."""
    S, Wn = len(rs), len(Ms)
    t = torch.full((Wn, S), -3.0, device="cuda")
    frame = dev(F)
    if kind == "plain":
        if dist is not None:
            frame = ctx.undistort_frame(frame, K, dist, out_mask=False)[0]
        win = ctx.search_grid(dev(rs), ctx.warp_stack(frame, Ms), t)
        return win, t.cpu().numpy(), None
    fmask = None if fm is None else dev(fm)
    if dist is not None:
        frame, fmask = ctx.undistort_frame(frame, K, dist, raw_mask=fmask)
    ws, wm = ctx.warp_stack_masked(frame, Ms, fmask)
    if kind == "masked":
        win = ctx.search_grid_masked(dev(rs), ws, wm, t)
        return win, t.cpu().numpy(), ctx.mask_counts(Wn)
    win = ctx.search_grid_covered(dev(rs), dev(rm), ws, wm, t)
    return win, t.cpu().numpy(), ctx.cover_counts(S * Wn)


def submit(ctx, st, kind, rs, rm, F, fm, Ms, block):
    S = len(rs)
    b = None if block is None else (0, S, 0, len(Ms))
    if kind == "plain":
        return st.submit(pin(rs), None if F is None else pin(F), Ms, block=b)
    if kind == "masked":
        return st.submit_masked(pin(rs), None if F is None else pin(F), None if fm is None else pin(fm), Ms, block=b)
    bm = ctx.pack_mask_bits(dev(rm)).cpu()
    return st.submit_covered(pin(rs), pin(bm), None if F is None else pin(F), None if fm is None else pin(fm), Ms, block=b)


@pytest.mark.parametrize("block", [False, True], ids=["whole", "block"])
@pytest.mark.parametrize("kind", ["plain", "masked", "covered"])
@pytest.mark.parametrize("shape", [(640, 480), (320, 240)], ids=["640x480", "320x240"])
def test_distorted_tickets_equal_the_chain(nmi, shape, kind, block):
    w, h = shape
    K = sy.intrinsics(w, h)
    F, rs, Ms = level(w, h, (3, 3, 1), (3, 3, 1), seed=5)
    F2, rs2, _ = level(w, h, (3, 3, 1), (3, 3, 1), seed=9)
    fm = hood(w, h) if kind != "plain" else None
    rm = render_masks(len(rs), w, h, 3) if kind == "covered" else None
    with nmi.NmiContext(w, h) as ctx, nmi.NmiStream(ctx, len(rs), len(Ms), depth=3) as st:
        st.keep_ratings()
        t_before = submit(ctx, st, kind, rs, rm, F, fm, Ms, None)   # submitted before the setting: not undistorted
        st.set_distortion(K, LENS)
        t1 = submit(ctx, st, kind, rs, rm, F, fm, Ms, block or None)
        t2 = submit(ctx, st, kind, rs2, rm, None, None, Ms, block or None)     # frame-less: the latest (distorted) warps
        results = [(t_before, None, rs, F), (t1, LENS, rs, F), (t2, LENS, rs2, F)]
        for t, dist, r, f in results:
            got = st.wait(t)
            ratings = st.ratings(t, len(Ms), len(r))
            win, ref_t, ref_n = standalone(ctx, kind, K, dist, f, fm, r, rm, Ms)
            assert got == win, (t, got, win)
            assert (bits(ratings) == bits(ref_t)).all()
            if ref_n is not None:
                assert (st.counts(t, ref_n.size) == ref_n.reshape(-1)).all()
        st.set_distortion(K, LENS)
        t3 = submit(ctx, st, kind, rs, rm, F2, fm, Ms, block or None)
        st.set_distortion(K, np.zeros(5))                                      # off: later tickets are undistorted
        t4 = submit(ctx, st, kind, rs, rm, F2, fm, Ms, block or None)
        for t, dist in ((t3, LENS), (t4, None)):
            got = st.wait(t)
            win, ref_t, _ = standalone(ctx, kind, K, dist, F2, fm, rs, rm, Ms)
            assert got == win and (bits(st.ratings(t, len(Ms), len(rs))) == bits(ref_t)).all()
        st.set_distortion(K, LENS)
        st.set_distortion(None, None)                                          # off again (NULL)
        t5 = submit(ctx, st, kind, rs, rm, F, fm, Ms, block or None)
        assert st.wait(t5) == standalone(ctx, kind, K, None, F, fm, rs, rm, Ms)[0]
