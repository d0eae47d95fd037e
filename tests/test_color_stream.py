"""Coloured and pitched keyframe streams on the GPU (-m gpu): nmi_stream_set_frame_format (include/nmi_hip.h).

Plain, masked and covered tickets (and their _block forms without a communicator) on pitched colour host frames equal grey
tickets on the frames the numpy twin converts (tests/helpers/color_np.py) -- winner, score bits, kept ratings, counts -- with and
without distortion.  A frame-less ticket in between reuses the latest warps; tickets submitted before the setting keep their
meaning; (GRAY, 0) gives the tickets of a stream that never had a format."""
import numpy as np
import pytest

from helpers import color_np as cnp
from helpers import undistort_np as unp
from orbslam2_nmi_amd import synthetic as sy
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


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def submit(ctx, st, kind, rs, rm, F, fm, Ms, block):
    """F: a pinned host frame in whatever layout the stream is set to (None: frame-less)."""
    S = len(rs)
    b = None if block is None else (0, S, 0, len(Ms))
    if kind == "plain":
        return st.submit(pin(rs), F, Ms, block=b)
    if kind == "masked":
        return st.submit_masked(pin(rs), F, None if fm is None else pin(fm), Ms, block=b)
    bm = ctx.pack_mask_bits(torch.from_numpy(rm).cuda()).cpu()
    return st.submit_covered(pin(rs), pin(bm), F, None if fm is None else pin(fm), Ms, block=b)


def outcome(st, t, Wn, S, kind):
    win = st.wait(t)
    r = st.ratings(t, Wn, S)
    n = st.counts(t, Wn if kind == "masked" else Wn * S) if kind != "plain" else None
    return win, r, n


def same(a, b):
    assert a[0] == b[0], (a[0], b[0])
    assert (bits(a[1]) == bits(b[1])).all()
    if a[2] is not None:
        assert (a[2] == b[2]).all()


@pytest.mark.parametrize("lens", ["none", "barrel"])
@pytest.mark.parametrize("block", [False, True], ids=["whole", "block"])
@pytest.mark.parametrize("kind", ["plain", "masked", "covered"])
@pytest.mark.parametrize("case", [(640, 480, cnp.RGB, 640 * 3 + 5), (322, 240, cnp.BGRA, 0)], ids=["640x480-rgb-pitched", "322x240-bgra"])
def test_colored_tickets_equal_grey_tickets(nmi, case, kind, block, lens):
    w, h, fmt, pitch = case
    K = sy.intrinsics(w, h)
    dist = LENS if lens == "barrel" else None
    F, rs, Ms = level(w, h, (3, 3, 1), (3, 3, 1), seed=5)
    F2, rs2, _ = level(w, h, (3, 3, 1), (3, 3, 1), seed=9)
    fm = hood(w, h) if kind != "plain" else None
    rm = render_masks(len(rs), w, h, 3) if kind == "covered" else None
    S, Wn = len(rs), len(Ms)
    C1, C2 = cnp.colorize(F, 1), cnp.colorize(F2, 2)
    H1, H2 = cnp.pack(C1, fmt, pitch, seed=1), cnp.pack(C2, fmt, pitch, seed=2)
    G1, G2 = cnp.to_gray(H1, fmt, w, h, pitch), cnp.to_gray(H2, fmt, w, h, pitch)
    b = block or None
    with nmi.NmiContext(w, h) as ctx, nmi.NmiStream(ctx, S, Wn, depth=4) as st, nmi.NmiStream(ctx, S, Wn, depth=4) as ref:
        st.keep_ratings()
        ref.keep_ratings()
        if dist is not None:
            st.set_distortion(K, dist)
            ref.set_distortion(K, dist)
        t_before = submit(ctx, st, kind, rs, rm, pin(G1), fm, Ms, None)       # grey, submitted before the setting
        st.set_frame_format(fmt, pitch)
        t1 = submit(ctx, st, kind, rs, rm, pin(H1), fm, Ms, b)
        t2 = submit(ctx, st, kind, rs2, rm, None, None, Ms, b)               # frame-less: the latest warps
        t3 = submit(ctx, st, kind, rs, rm, pin(H2), fm, Ms, b)
        r_before = submit(ctx, ref, kind, rs, rm, pin(G1), fm, Ms, None)
        r1 = submit(ctx, ref, kind, rs, rm, pin(G1), fm, Ms, b)
        r2 = submit(ctx, ref, kind, rs2, rm, None, None, Ms, b)
        r3 = submit(ctx, ref, kind, rs, rm, pin(G2), fm, Ms, b)
        for t, r, s in ((t_before, r_before, S), (t1, r1, S), (t2, r2, len(rs2)), (t3, r3, S)):
            same(outcome(st, t, Wn, s, kind), outcome(ref, r, Wn, s, kind))
        st.set_frame_format(cnp.GRAY, 0)                                    # off: later frames are dense grey again
        t4 = submit(ctx, st, kind, rs, rm, pin(G2), fm, Ms, b)
        r4 = submit(ctx, ref, kind, rs, rm, pin(G2), fm, Ms, b)
        same(outcome(st, t4, Wn, S, kind), outcome(ref, r4, Wn, S, kind))


def test_stream_format_switches_and_rejections(nmi):
    """A pitched grey frame, then a wider format (the colour slots grow), then back; rejected settings leave the stream as it was."""
    w, h = 320, 240
    F, rs, Ms = level(w, h, (3, 1, 1), (3, 1, 1), seed=3)
    S, Wn = len(rs), len(Ms)
    C1 = cnp.colorize(F, 4)
    layouts = [(cnp.GRAY, w + 3, F), (cnp.RGB, 0, C1), (cnp.RGBA, w * 4 + 16, C1), (cnp.BGR, w * 3 + 1, C1)]
    with nmi.NmiContext(w, h) as ctx, nmi.NmiStream(ctx, S, Wn, depth=2) as st, nmi.NmiStream(ctx, S, Wn, depth=2) as ref:
        for k, (fmt, pitch, img) in enumerate(layouts):
            st.set_frame_format(fmt, pitch)
            for bad in ((7, 0), (fmt, 1), (fmt, -1)):
                with pytest.raises(nmi.capi.NmiError):
                    st.set_frame_format(*bad)
            H = cnp.pack(img, fmt, pitch, seed=k)
            G = cnp.to_gray(H, fmt, w, h, pitch)
            t = st.submit(pin(rs), pin(H), Ms)
            r = ref.submit(pin(rs), pin(G), Ms)
            assert st.wait(t) == ref.wait(r), (fmt, pitch)
