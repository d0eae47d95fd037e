"""Keyframe streams fed full-size host frames on the GPU (-m gpu): nmi_stream_set_frame_reduction (include/nmi_hip.h).

Plain, masked and covered tickets (and their _block forms without a communicator) on pitched full-size host frames equal grey
tickets on the frames the numpy twin reduces (tests/helpers/reduce_np.py) -- winner, score bits, kept ratings, counts -- with and
without distortion.  A frame-less ticket in between reuses the latest warps; tickets submitted before the setting keep their
meaning; (1, GRAY, 0) gives the tickets of a stream that never had a setting; of set_frame_format and set_frame_reduction the
later call wins."""
import numpy as np
import pytest

from helpers import color_np as cnp
from helpers import reduce_np as rnp
from helpers import undistort_np as unp
from orbslam2_nmi_amd import synthetic as sy
from test_color_stream import outcome, same, submit
from test_reduce_level import full_size
from test_stream_masked import hood, level, pin, render_masks

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

LENS = unp.FAMILIES["barrel"]


@pytest.fixture(scope="module")
def nmi():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    import orbslam2_nmi_amd as m
    m.load_library()
    return m


def host_frame(F, f, fmt, pitch, seed):
    """The search-size grey frame F at f times its size, in fmt with a pitch -> (flat host buffer, the twin's reduced frame)."""
    big = full_size(F, f, seed)
    img = big if fmt == cnp.GRAY else cnp.colorize(big, seed)
    buf = cnp.pack(img, fmt, pitch, seed=seed)
    h, w = F.shape
    return buf, rnp.reduce_frame(buf, fmt, w, h, f, pitch)


CASES = [(320, 240, 2, cnp.RGB, 640 * 3 + 5), (212, 120, 4, cnp.GRAY, 0), (322, 240, 3, cnp.BGRA, 966 * 4 + 64)]


@pytest.mark.parametrize("lens", ["none", "barrel"])
@pytest.mark.parametrize("block", [False, True], ids=["whole", "block"])
@pytest.mark.parametrize("kind", ["plain", "masked", "covered"])
@pytest.mark.parametrize("case", CASES, ids=["320x240-f2-rgb-pitched", "212x120-f4-gray", "322x240-f3-bgra-pitched"])
def test_reduced_tickets_equal_grey_tickets(nmi, case, kind, block, lens):
    w, h, f, fmt, pitch = case
    K = sy.intrinsics(w, h)
    dist = LENS if lens == "barrel" else None
    F, rs, Ms = level(w, h, (3, 3, 1), (3, 3, 1), seed=5)
    F2, rs2, _ = level(w, h, (3, 3, 1), (3, 3, 1), seed=9)
    fm = hood(w, h) if kind != "plain" else None                           # dense [H][W], at the search size
    rm = render_masks(len(rs), w, h, 3) if kind == "covered" else None
    S, Wn = len(rs), len(Ms)
    H1, G1 = host_frame(F, f, fmt, pitch, 1)
    H2, G2 = host_frame(F2, f, fmt, pitch, 2)
    assert G1.shape == (h, w) and (G1 != G2).any()
    b = block or None
    with nmi.NmiContext(w, h) as ctx, nmi.NmiStream(ctx, S, Wn, depth=4) as st, nmi.NmiStream(ctx, S, Wn, depth=4) as ref:
        st.keep_ratings()
        ref.keep_ratings()
        if dist is not None:
            st.set_distortion(K, dist)
            ref.set_distortion(K, dist)
        t_before = submit(ctx, st, kind, rs, rm, pin(G1), fm, Ms, None)       # grey, submitted before the setting
        st.set_frame_reduction(f, fmt, pitch)
        t1 = submit(ctx, st, kind, rs, rm, pin(H1), fm, Ms, b)
        t2 = submit(ctx, st, kind, rs2, rm, None, None, Ms, b)               # frame-less: the latest warps
        t3 = submit(ctx, st, kind, rs, rm, pin(H2), fm, Ms, b)
        r_before = submit(ctx, ref, kind, rs, rm, pin(G1), fm, Ms, None)
        r1 = submit(ctx, ref, kind, rs, rm, pin(G1), fm, Ms, b)
        r2 = submit(ctx, ref, kind, rs2, rm, None, None, Ms, b)
        r3 = submit(ctx, ref, kind, rs, rm, pin(G2), fm, Ms, b)
        for t, r, s in ((t_before, r_before, S), (t1, r1, S), (t2, r2, len(rs2)), (t3, r3, S)):
            same(outcome(st, t, Wn, s, kind), outcome(ref, r, Wn, s, kind))
        st.set_frame_reduction(1, cnp.GRAY, 0)                              # off: later frames are dense grey again
        t4 = submit(ctx, st, kind, rs, rm, pin(G2), fm, Ms, b)
        r4 = submit(ctx, ref, kind, rs, rm, pin(G2), fm, Ms, b)
        same(outcome(st, t4, Wn, S, kind), outcome(ref, r4, Wn, S, kind))


def test_stream_settings_switch_and_rejections(nmi):
    """A factor, a larger factor (the slots grow), a colour frame of the search size through set_frame_format (the later call wins),
    back to a factor; rejected settings leave the stream as it was."""
    w, h = 160, 120
    F, rs, Ms = level(w, h, (3, 1, 1), (3, 1, 1), seed=3)
    S, Wn = len(rs), len(Ms)
    settings = [(2, cnp.GRAY, 2 * w + 3), (4, cnp.RGB, 0), (1, cnp.RGBA, w * 4 + 16), (3, cnp.BGR, 3 * w * 3 + 1), (1, cnp.GRAY, 0)]
    with nmi.NmiContext(w, h) as ctx, nmi.NmiStream(ctx, S, Wn, depth=2) as st, nmi.NmiStream(ctx, S, Wn, depth=2) as ref:
        for k, (f, fmt, pitch) in enumerate(settings):
            if f == 1:
                st.set_frame_format(fmt, pitch)
            else:
                st.set_frame_reduction(f, fmt, pitch)
            for bad in ((0, fmt, pitch), (5, fmt, pitch), (f, 7, 0), (f, fmt, 1), (f, fmt, -1)):
                with pytest.raises(nmi.capi.NmiError):
                    st.set_frame_reduction(*bad)
            H, G = host_frame(F, f, fmt, pitch, k)
            t = st.submit(pin(rs), pin(H), Ms)
            r = ref.submit(pin(rs), pin(G), Ms)
            assert st.wait(t) == ref.wait(r), (f, fmt, pitch)
