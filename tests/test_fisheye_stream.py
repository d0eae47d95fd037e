"""Fisheye keyframe streams on the GPU (-m gpu): nmi_stream_set_distortion_fisheye (include/nmi_hip.h).

Plain, masked and covered tickets (and their _block forms without a communicator) on raw frames equal the standalone chain
nmi_undistort_frame_fisheye -> nmi_warp_stack[_masked] -> nmi_search_grid[_masked / _covered]: winner, score bits, kept
rating tables, counts.  A stream has one lens setting: a later nmi_stream_set_distortion (radial-tangential) replaces the
fisheye one, and NULL through either setter turns it off."""
import numpy as np
import pytest

from helpers import fisheye_np as fnp
from helpers import undistort_np as unp
from orbslam2_nmi_amd import synthetic as sy
from test_stream_masked import hood, level, render_masks
from test_undistort_stream import bits, standalone, submit

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

LENS = fnp.FAMILIES["strong"]
RADTAN = unp.FAMILIES["pincushion"]


@pytest.fixture(scope="module")
def nmi():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    import orbslam2_nmi_amd as m
    m.load_library()
    return m


@pytest.mark.parametrize("block", [False, True], ids=["whole", "block"])
@pytest.mark.parametrize("kind", ["plain", "masked", "covered"])
@pytest.mark.parametrize("shape", [(640, 480), (333, 97)], ids=["640x480", "333x97"])
def test_fisheye_tickets_equal_the_chain(nmi, shape, kind, block):
    w, h = shape
    K = sy.intrinsics(w, h)
    Kr = fnp.pinhole_K(K, 1 / 0.6)
    Kr[0, 2] += 0.02 * w
    F, rs, Ms = level(w, h, (3, 3, 1), (3, 3, 1), seed=5)
    F2, rs2, _ = level(w, h, (3, 3, 1), (3, 3, 1), seed=9)
    fm = hood(w, h) if kind != "plain" else None
    rm = render_masks(len(rs), w, h, 3) if kind == "covered" else None
    b = block or None
    with nmi.NmiContext(w, h) as ctx, nmi.NmiStream(ctx, len(rs), len(Ms), depth=5) as st:
        fctx = fnp.FisheyeCtx(ctx, Kr)
        st.keep_ratings()
        t_before = submit(ctx, st, kind, rs, rm, F, fm, Ms, None)   # submitted before the setting: not undistorted
        st.set_distortion_fisheye(K, Kr, LENS)
        t1 = submit(ctx, st, kind, rs, rm, F, fm, Ms, b)
        t2 = submit(ctx, st, kind, rs2, rm, None, None, Ms, b)      # frame-less: the latest (undistorted) warps
        for t, c, dist, r in ((t_before, ctx, None, rs), (t1, fctx, LENS, rs), (t2, fctx, LENS, rs2)):
            got = st.wait(t)
            ratings = st.ratings(t, len(Ms), len(r))
            win, ref_t, ref_n = standalone(c, kind, K, dist, F, fm, r, rm, Ms)
            assert got == win, (t, got, win)
            assert (bits(ratings) == bits(ref_t)).all()
            if ref_n is not None:
                assert (st.counts(t, ref_n.size) == ref_n.reshape(-1)).all()
        st.set_distortion(K, RADTAN)                                # the later call wins: radial-tangential
        t3 = submit(ctx, st, kind, rs, rm, F2, fm, Ms, b)
        st.set_distortion_fisheye(K, Kr, LENS)                      # ... and back
        t4 = submit(ctx, st, kind, rs, rm, F2, fm, Ms, b)
        st.set_distortion_fisheye(None, None, None)                 # off (NULL): later tickets are undistorted
        t5 = submit(ctx, st, kind, rs, rm, F2, fm, Ms, b)
        st.set_distortion_fisheye(K, None, np.zeros(4))             # four zeros, K_raw = K: an ideal equidistant lens, on
        t6 = submit(ctx, st, kind, rs, rm, F2, fm, Ms, b)
        st.set_distortion(None, None)                               # off through the other setter
        t7 = submit(ctx, st, kind, rs, rm, F2, fm, Ms, b)
        zero = fnp.FisheyeCtx(ctx, None)
        seen = {}
        for t, c, dist in ((t3, ctx, RADTAN), (t4, fctx, LENS), (t5, ctx, None), (t6, zero, np.zeros(4)), (t7, ctx, None)):
            got = st.wait(t)
            win, ref_t, _ = standalone(c, kind, K, dist, F2, fm, rs, rm, Ms)
            assert got == win and (bits(st.ratings(t, len(Ms), len(rs))) == bits(ref_t)).all(), t
            seen[t] = ref_t
        assert (bits(seen[t3]) != bits(seen[t4])).any() and (bits(seen[t5]) != bits(seen[t6])).any()   # the settings differ
        assert (bits(seen[t5]) == bits(seen[t7])).all()
