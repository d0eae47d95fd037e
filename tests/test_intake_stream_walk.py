"""GPU test (-m gpu) of every move between a stream's intake settings while earlier tickets are still running
(nmi_stream_set_distortion[_fisheye], _set_frame_format, _set_frame_reduction, _set_tone_map).

The states and the Euler circuit are walk F's (tests/test_intake_level_walk.py): 27 states of (lens, frame), 270 directed
moves, per layout of tests/helpers/intake_np.py.  ONE stream of depth 4 with kept ratings makes one ticket per move: the
move's setter calls, then a freshly packed host frame read in the new format, its content rolled for every ticket.  The kind
cycles plain -> masked -> covered per ticket; every seventh ticket is frame-less (the latest warps); every eleventh uses the
block form.  A ticket is collected only when its slot is needed, so every setter call -- and with it every change of d_color's
size, of d_ud / d_ud_mask, of d_frame's use as scratch and of the one shared tone work -- happens with three tickets in flight.

The reference is a second stream that never gets an intake setting: its frames and frame masks are grey_of(...) of the same
host bytes, computed on the CPU; renders, render masks and homographies are the same.  For every ticket the winner, the
ratings' bits and the counts must be equal (the outcome / same harness of tests/test_color_stream.py; the submissions follow
its submit(), with the render masks' bits packed once: packing them on the device per ticket would wait for the tickets in
flight).  Refused setter calls between tickets leave the later tickets unchanged.

A frame-less masked or covered ticket needs a latest frame that was submitted with masks; where the cycle would put one behind
a plain frame, that ticket is a plain one."""
import pytest

from helpers import color_np as cnp
from helpers import intake_np as inp
from helpers import tone_np as tnp
from helpers import walk_plan as wp
from orbslam2_nmi_amd import capi
from orbslam2_nmi_amd import synthetic as sy
from test_color_stream import outcome, same
from test_stream_masked import hood, level, packbits, pin, render_masks

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

KINDS = ("plain", "masked", "covered")
S, WN, DEPTH = 3, 3, 4
START = ("none", "gray")


@pytest.fixture(scope="module")
def nmi():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    import orbslam2_nmi_amd as m
    m.load_library()
    return m


def submit(st, kind, rs, bm, F, fm, Ms, block):
    """One ticket.  rs, bm, F: pinned host tensors (F None: frame-less); fm: a numpy frame mask or None."""
    b = (0, S, 0, WN) if block else None
    if kind == "plain":
        return st.submit(rs, F, Ms if F is not None else None, block=b)
    mask = None if fm is None else pin(fm)
    if kind == "masked":
        return st.submit_masked(rs, F, mask, Ms if F is not None else None, block=b)
    return st.submit_covered(rs, bm, F, mask, Ms if F is not None else None, block=b)


class StreamWalk:
    """The walking stream's setters by axis, with the tone map it currently holds."""

    def __init__(self, st, lay, K, origin):
        self.st, self.lay, self.K, self.Kr, self.origin, self.tone = st, lay, K, inp.raw_K(K, lay.w), origin, "shift"

    def set_lens(self, lens):
        if lens == "none":
            self.st.set_distortion(None, None)
        elif lens == "barrel":
            self.st.set_distortion(self.K, inp.BARREL)
        else:
            self.st.set_distortion_fisheye(self.K, self.Kr, inp.FISHEYE)

    def set_format(self, frame):
        factor, fmt, _ = inp.frame_spec(frame)
        if frame == "off":
            self.st.set_frame_reduction(1, cnp.GRAY, 0)
        elif factor == 1:
            self.st.set_frame_format(fmt, self.lay.pitch)
        else:
            self.st.set_frame_reduction(factor, fmt, self.lay.pitch)

    def set_tone(self, tone):
        self.st.set_tone_map(None if tone == "shift" else tnp.capi_tone(capi, inp.TONES[tone]))
        self.tone = tone

    def move_frame(self, src, dst, i):
        """As the level walk's: one call, the tone map alone, or the two calls in the order of the move's number."""
        fs, fd = inp.frame_spec(src), inp.frame_spec(dst)
        if fd[2] is None:
            self.set_format(dst)
        elif fs[2] is not None and fs[0] == fd[0]:
            self.set_tone(fd[2])
        elif inp.call_order(i, self.origin) == "tone-first":
            self.set_tone(fd[2])
            self.set_format(dst)
        else:
            self.set_format(dst)
            self.set_tone(fd[2])

    def refuse(self, what):
        skew = self.K.copy()
        skew[0, 1] = 0.5
        with pytest.raises(capi.NmiError):
            if "tone map" in what:
                self.st.set_tone_map(capi.ToneMap(mode=capi.TONE_PERCENTILE, bits=16, p_lo=5000, p_hi=5000))
            elif "GRAY16" in what:
                self.st.set_frame_format(capi.FRAME_GRAY16, self.lay.pitch + 1)
            elif "Bayer" in what:
                self.st.set_frame_format(capi.FRAME_BAYER_GRBG, self.lay.w - 1)
            else:
                self.st.set_distortion_fisheye(skew, self.Kr, inp.FISHEYE)


@pytest.mark.parametrize("layout", list(inp.LAYOUTS))
def test_one_stream_walks_every_move_between_its_intakes(nmi, layout):
    lay = inp.LAYOUTS[layout]
    w, h = lay.w, lay.h
    axes = (inp.LENSES, inp.FRAME_NAMES)
    edges = wp.check_circuit(wp.euler_circuit(START, axes), START, axes)
    assert len(edges) == 270
    deep_at = next(i for i, (_, d) in enumerate(edges) if i >= 30 and inp.is_deep(d[1]))
    flat_at = next(i for i, (_, d) in enumerate(edges) if i >= 75 and not inp.is_deep(d[1]))
    refusals = {deep_at: "a bad tone map in a deep state", flat_at: "a bad tone map in a non-deep state", 120: "an odd pitch for GRAY16",
                165: "a Bayer pitch below the width", 210: "a skewed K for the fisheye setter"}
    assert len(refusals) == 5
    K = sy.intrinsics(w, h)
    scenes = [level(w, h, (3, 1, 1), (3, 1, 1), seed=s) for s in (5, 9)]
    Ms = scenes[0][2]
    stacks = [pin(sc[1]) for sc in scenes]
    assert stacks[0].shape[0] == S and len(Ms) == WN
    fm = hood(w, h)
    bm = pin(packbits(render_masks(S, w, h, 3)))
    base = inp.walk_buffer(lay)
    with nmi.NmiContext(w, h) as ctx, nmi.NmiStream(ctx, S, WN, depth=DEPTH) as st, nmi.NmiStream(ctx, S, WN, depth=DEPTH) as ref:
        st.keep_ratings()
        ref.keep_ratings()
        wk = StreamWalk(st, lay, K, origin=0 if layout == "A" else 1)
        pending, framed, compared = [], {"kind": None}, []

        def collect():
            name, t, r, kind = pending.pop(0)
            try:
                same(outcome(st, t, WN, S, kind), outcome(ref, r, WN, S, kind))
            except AssertionError as e:
                raise AssertionError(f"{name} ({kind}) differs from the ticket on the twin's frame: {e}") from e
            compared.append(name)

        def ticket(name, k, state, kind, frameless=False, block=False):
            """Ticket k in `state`: on the walking stream the raw bytes, on the reference the twin's grey frame and mask."""
            if len(pending) == DEPTH:          # its slot is needed now (submitted after the setter calls: three were in flight)
                raise AssertionError("collect before the setter calls")
            rs = stacks[k % 2]
            if frameless:
                if kind != "plain" and framed["kind"] == "plain":
                    kind = "plain"             # the latest frame made no masks
                t = submit(st, kind, rs, bm, None, None, Ms, block)
                r = submit(ref, kind, rs, bm, None, None, Ms, block)
            else:
                host = inp.rolled(base, lay, k)
                raw_mask = fm if kind != "plain" else None
                grey, mask = inp.grey_of(host, w, h, lay.pitch, lay.off, state, raw_mask, K=K)
                F = pin(host)[lay.off:] if state[1] != "off" else pin(host[lay.off:lay.off + w * h])
                t = submit(st, kind, rs, bm, F, raw_mask, Ms, block)
                r = submit(ref, kind, rs, bm, pin(grey), mask if kind != "plain" else None, Ms, block)
                framed["kind"] = kind
            pending.append((name, t, r, kind))

        ticket("as created", 1000, ("none", "off"), "plain")
        wk.set_format(START[1])
        ticket("at the start", 1001, START, "masked")
        for i, (src, dst) in enumerate(edges):
            if len(pending) == DEPTH:
                collect()
            assert len(pending) == min(i + 2, DEPTH - 1)       # the setters below are called with these in flight
            if src[0] != dst[0]:
                wk.set_lens(dst[0])
            else:
                wk.move_frame(src[1], dst[1], i)
            if i in refusals:
                wk.refuse(refusals[i])
            ticket(f"move {i} {src} -> {dst}", i, dst, KINDS[i % 3], frameless=i % 7 == 6, block=i % 11 == 10)
        if len(pending) == DEPTH:
            collect()
        wk.set_format("off")                                   # off again; the tone map stays set
        ticket("everything off again", 1002, ("none", "off"), "covered")
        while pending:
            collect()
        assert len(compared) == 270 + 3
