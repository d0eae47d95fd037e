"""GPU tests (-m gpu) of the valid range of keyframe streams (nmi_stream_set_valid_range, include/nmi_hip.h), S = 3, Wn = 3.

On a stream with set_frame_reduction(f, FRAME_GRAY16, pitch), a tone map and the range, every ticket equals the same submission on
a plain-grey stream given the numpy twin's frame and the twin's validity mask (tests/helpers/valid_np.py: deep_frame): winner,
score bits, kept ratings and nmi_stream_copy_counts.  The frames are tests/helpers/valid_pipeline_cases.py's, whose premises
tests/test_valid_pipeline_plan.py checks on the CPU."""
import numpy as np
import pytest

from helpers import tone_np as tnp
from helpers import undistort_np as unp
from helpers import valid_np as vnp
from helpers import valid_pipeline_cases as cases
from orbslam2_nmi_amd import capi, synthetic as sy
from test_color_stream import outcome, same, submit
from test_stream_masked import level, pin, render_masks

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

S, WN = 3, 3
RANGE = cases.RANGE
LENS = unp.FAMILIES["barrel"]
E = capi.ERR_INVALID_ARGUMENT


@pytest.fixture(scope="module")
def nmi():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    import orbslam2_nmi_amd as m
    m.load_library()
    return m


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


class Frames:
    """Three search levels around synthetic scenes, their camera frames as planted pipeline frames at factor f."""

    def __init__(self, w, h, f):
        self.w, self.h, self.f = w, h, f
        self.pitch = 2 * f * w + 6
        self.levels = [level(w, h, (3, 1, 1), (3, 1, 1), seed=s) for s in (5, 9, 11)]
        self.Ms = self.levels[0][2]
        self.px = [cases.frame(F, f, s) for (F, _, _), s in zip(self.levels, (5, 9, 11))]
        for px in self.px:
            cases.premises(px, f)
        self.rs = [rs for _, rs, _ in self.levels]

    def host(self, k):
        return pin(tnp.pack16(self.px[k], self.pitch, seed=k))

    def twin(self, k, tm, rng, fm=None):
        """(grey frame, validity mask ANDed with fm) of frame k, pinned."""
        gray, mask = vnp.deep_frame(self.px[k], self.f, tm, rng, fm)
        return pin(gray), mask


def streams(nmi, ctx, fr, tm, depth=4, lens=False):
    st, ref = nmi.NmiStream(ctx, S, WN, depth=depth), nmi.NmiStream(ctx, S, WN, depth=depth)
    for s in (st, ref):
        s.keep_ratings()
        if lens:
            s.set_distortion(sy.intrinsics(fr.w, fr.h), LENS)
    st.set_frame_reduction(fr.f, capi.FRAME_GRAY16, fr.pitch)
    st.set_tone_map(cases.capi_tone(capi, tm))
    return st, ref


@pytest.mark.parametrize("mode", list(cases.tone_maps()))
@pytest.mark.parametrize("kind", ["masked", "covered"])
@pytest.mark.parametrize("size,f", [((64, 48), 1), ((54, 38), 2), ((52, 38), 1)], ids=["64x48", "54x38-f2", "52x38"])
def test_ranged_tickets_equal_grey_tickets_with_the_twins_mask(nmi, size, f, kind, mode):
    """With and without h_frame_mask, whole and _block forms, a frame-less ticket in between that reuses the ranged frame's warp masks;
    and the range changes the ticket."""
    w, h = size
    tm = cases.tone_maps()[mode]
    fr = Frames(w, h, f)
    fm = cases.hood(w, h)
    rm = render_masks(S, w, h, 3) if kind == "covered" else None
    with nmi.NmiContext(w, h) as ctx:
        st, ref = streams(nmi, ctx, fr, tm)
        with st, ref:
            st.set_valid_range(*RANGE)
            pairs = []
            for k, (mask, block) in enumerate(((None, None), (fm, True), (fm, None))):
                gray, vm = fr.twin(k, tm, RANGE, mask)
                t = submit(ctx, st, kind, fr.rs[k], rm, fr.host(k), mask, fr.Ms, block)
                r = submit(ctx, ref, kind, fr.rs[k], rm, gray, vm, fr.Ms, block)
                pairs.append((t, r))
                if k == 0:                                             # frame-less: the ranged frame's warps and warp masks
                    pairs.append((submit(ctx, st, kind, fr.rs[1], rm, None, None, fr.Ms, None),
                                  submit(ctx, ref, kind, fr.rs[1], rm, None, None, fr.Ms, None)))
            got = [(outcome(st, t, WN, S, kind), outcome(ref, r, WN, S, kind)) for t, r in pairs]
            for a, b in got:
                same(a, b)
            st.set_valid_range()                                       # off: the same frame is another ticket
            t = submit(ctx, st, kind, fr.rs[0], rm, fr.host(0), None, fr.Ms, None)
            gray, _ = fr.twin(0, tm, vnp.OFF)
            r = submit(ctx, ref, kind, fr.rs[0], rm, gray, None, fr.Ms, None)
            plain = outcome(st, t, WN, S, kind)
            same(plain, outcome(ref, r, WN, S, kind))
            assert (bits(plain[1]) != bits(got[0][0][1])).any()


def test_two_frames_in_flight_and_a_third_in_the_first_slot(nmi):
    """Depth 2: two different ranged frames in flight, then a third that reuses the first ticket slot and the first frame buffer,
    whose frame-mask slot the second-to-last conversion wrote on the compute stream.  Each equals its own baseline."""
    w, h = 64, 48
    tm = cases.tone_maps()["equalize"]
    fr = Frames(w, h, 1)
    fm = cases.hood(w, h)
    masks = (fm, None, np.ascontiguousarray(fm[:, ::-1]))              # uploaded, validity alone, another upload over the slot
    with nmi.NmiContext(w, h) as ctx:
        st, ref = streams(nmi, ctx, fr, tm, depth=2)
        with st, ref:
            st.set_valid_range(*RANGE)
            twins = [fr.twin(k, tm, RANGE, masks[k]) for k in range(3)]
            ta = submit(ctx, st, "masked", fr.rs[0], None, fr.host(0), masks[0], fr.Ms, None)
            tb = submit(ctx, st, "masked", fr.rs[1], None, fr.host(1), masks[1], fr.Ms, None)
            a = outcome(st, ta, WN, S, "masked")
            tc = submit(ctx, st, "masked", fr.rs[2], None, fr.host(2), masks[2], fr.Ms, None)
            b = outcome(st, tb, WN, S, "masked")
            c = outcome(st, tc, WN, S, "masked")
            want = []
            for k in range(3):
                r = submit(ctx, ref, "masked", fr.rs[k], None, twins[k][0], twins[k][1], fr.Ms, None)
                want.append(outcome(ref, r, WN, S, "masked"))
            for got, exp in zip((a, b, c), want):
                same(got, exp)
            assert (bits(a[1]) != bits(c[1])).any()


@pytest.mark.parametrize("mode", ["shift", "equalize", "clahe3x2"])
def test_a_plain_ticket_takes_the_statistics_only(nmi, mode):
    w, h = 54, 38
    tm = cases.tone_maps()[mode]
    fr = Frames(w, h, 2)
    with nmi.NmiContext(w, h) as ctx:
        st, ref = streams(nmi, ctx, fr, tm)
        with st, ref:
            t_off = st.submit(pin(fr.rs[0]), fr.host(0), fr.Ms)       # submitted before the setting: not affected
            st.set_valid_range(*RANGE)
            t_on = st.submit(pin(fr.rs[0]), fr.host(0), fr.Ms)
            r_off = ref.submit(pin(fr.rs[0]), fr.twin(0, tm, vnp.OFF)[0], fr.Ms)
            r_on = ref.submit(pin(fr.rs[0]), fr.twin(0, tm, RANGE)[0], fr.Ms)
            off, on = outcome(st, t_off, WN, S, "plain"), outcome(st, t_on, WN, S, "plain")
            same(off, outcome(ref, r_off, WN, S, "plain"))
            same(on, outcome(ref, r_on, WN, S, "plain"))
            if mode == "shift":                                        # no statistics: the same grey bytes
                assert (bits(off[1]) == bits(on[1])).all()
            else:
                assert (bits(off[1]) != bits(on[1])).any()


@pytest.mark.parametrize("kind", ["masked", "covered"])
def test_a_lens_undistorts_the_validity_mask(nmi, kind):
    w, h = 64, 48
    tm = cases.tone_maps()["pct"]
    fr = Frames(w, h, 1)
    fm = cases.hood(w, h)
    rm = render_masks(S, w, h, 3) if kind == "covered" else None
    with nmi.NmiContext(w, h) as ctx:
        st, ref = streams(nmi, ctx, fr, tm, lens=True)
        with st, ref:
            st.set_valid_range(*RANGE)
            pairs = []
            for k, mask in enumerate((None, fm)):
                gray, vm = fr.twin(k, tm, RANGE, mask)
                pairs.append((submit(ctx, st, kind, fr.rs[k], rm, fr.host(k), mask, fr.Ms, None),
                              submit(ctx, ref, kind, fr.rs[k], rm, gray, vm, fr.Ms, None)))
            for t, r in pairs:
                same(outcome(st, t, WN, S, kind), outcome(ref, r, WN, S, kind))


def test_the_setting_holds_for_later_submissions_only(nmi):
    """Set between two submissions: the earlier ticket, still in flight, is the unranged one.  Refused arguments and a NULL stream
    leave the setting as it was; under plain grey frames the range is kept and ignored."""
    w, h = 52, 38
    tm = cases.tone_maps()["equalize"]
    fr = Frames(w, h, 1)
    with nmi.NmiContext(w, h) as ctx:
        lib = ctx._lib
        st, ref = streams(nmi, ctx, fr, tm)
        with st, ref:
            t0 = st.submit_masked(pin(fr.rs[0]), fr.host(0), None, fr.Ms)
            st.set_valid_range(*RANGE)
            for lo, hi in ((-1, 5), (7, 3), (0, 65536)):
                assert lib.nmi_stream_set_valid_range(st._h, lo, hi) == E, (lo, hi)
                with pytest.raises(capi.NmiError):
                    st.set_valid_range(lo, hi)
            assert lib.nmi_stream_set_valid_range(None, *RANGE) == E
            t1 = st.submit_masked(pin(fr.rs[0]), fr.host(0), None, fr.Ms)
            r0 = ref.submit_masked(pin(fr.rs[0]), fr.twin(0, tm, vnp.OFF)[0], None, fr.Ms)
            gray, vm = fr.twin(0, tm, RANGE)
            r1 = ref.submit_masked(pin(fr.rs[0]), gray, pin(vm), fr.Ms)
            a, b = outcome(st, t0, WN, S, "masked"), outcome(st, t1, WN, S, "masked")
            same(a, outcome(ref, r0, WN, S, "masked"))
            same(b, outcome(ref, r1, WN, S, "masked"))
            assert (bits(a[1]) != bits(b[1])).any() and (a[2] != b[2]).any()
            st.set_frame_format(capi.FRAME_GRAY, 0)                    # not deep: the range is kept, and ignored
            t2 = st.submit_masked(pin(fr.rs[1]), gray, None, fr.Ms)
            r2 = ref.submit_masked(pin(fr.rs[1]), gray, None, fr.Ms)
            same(outcome(st, t2, WN, S, "masked"), outcome(ref, r2, WN, S, "masked"))
