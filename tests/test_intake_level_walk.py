"""GPU test (-m gpu) of every move between a level's intake settings, across the families: colour, raw sensor and deep frames,
reduced or not, under no lens, a radial-tangential lens and a fisheye lens (nmi_level_set_distortion[_fisheye],
_set_frame_format, _set_frame_reduction, _set_tone_map), with the harness of tests/test_level_settings_walk.py.

Walk F (frame x lens; the kind -- plain, masked or covered -- fixed per test): 27 states of (lens, frame), nine readings of
ONE byte buffer (tests/helpers/intake_np.py), 10 moves out of each: 270 directed moves on one Euler circuit, walked by ONE
level.  A lens move is one call.  A frame move into a deep value is two: the tone map first, while the format still ignores it,
or the format first, which passes through the deep format under the tone map set before (compared there too); which of the two
goes by the move's number (intake_np.call_order; masked walks number from 1, so that between the kinds every such move is made
both ways).  Between two deep values of one factor it is nmi_level_set_tone_map alone; leaving a deep value leaves the tone
map set.  After every move the level is run and compared byte for byte -- winner, score, renders, warps, ratings, masks and
counts -- with a fresh level put straight into that state.  What this pins is the lifetime of d_ud, d_ud_mask, d_small and the
tone work across families: Bayer + lens (two nodes) -> RGB + lens (one fused node) -> GRAY16 EQUALIZE + lens (histogram, table,
conversion and undistortion nodes); EQUALIZE -> WINDOW -> EQUALIZE over the cached fixed table; deep -> not deep -> deep, where
the tone work is dropped and rebuilt; radial-tangential -> fisheye under a reduced frame.

Walk K (kind x lens; the frame -- grbg, deep-eq or deep-pct-f2 -- fixed per test): 9 states, 36 moves, masked <-> covered two
calls, off then on: d_ud_mask comes and goes beside d_small and the tone work.

Tie to the twins: byte equality with another level would pass if every level were wrong alike, so each cached reference is
checked once against the CPU twins: its warps (and warp masks) are nmi_warp_stack[_masked] of grey_of(...) uploaded as a plain
grey frame with its mask, and its winner and ratings those of the standalone search on them (test_reduce_level.rest_of_chain).

Refused calls at fixed points of walk F -- a bad tone map in a deep and in a non-deep state, an odd pitch for GRAY16, a Bayer
pitch below the width, a skewed K for the fisheye setter -- leave the level equal to its state's reference.

tests/test_intake_walk_plan.py shows, without a GPU, that the 27 frames (and those passed through) are pairwise different."""
from types import SimpleNamespace

import pytest

from helpers import color_np as cnp
from helpers import intake_np as inp
from helpers import tone_np as tnp
from helpers import walk_plan as wp
from orbslam2_nmi_amd import capi
from test_color_level import bits, lens_K
from test_covered_level import CoveredScene
from test_fisheye_level import raw_K
from test_level_settings_walk import Walk
from test_masked_level import dev, views, warps
from test_reduce_level import rest_of_chain

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

KINDS = ("plain", "masked", "covered")
S, WN = 3, 3
OFF = ("plain", "none", "off")
START = ("none", "gray")


@pytest.fixture(scope="module")
def nmi():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    import orbslam2_nmi_amd as m
    m.load_library()
    return m


class IntakeWalk(Walk):
    """Walk on the intake walks' buffer: a state is (kind, lens, frame), frame a name of intake_np (one of the nine, "off", or a
    deep reading passed through).  snapshot, check and set_kind are the existing walk's."""

    def __init__(self, nmi, ctx, lay, origin=0):
        self.nmi, self.ctx, self.S, self.Wn, self.lay, self.origin = nmi, ctx, S, WN, lay, origin
        self.sc = CoveredScene(nmi, ctx, lay.w, lay.h, lay.mesh)
        self.K = lens_K(self.sc.rp)
        self.Kr = inp.raw_K(self.K, lay.w)
        assert (self.Kr == raw_K(self.K, lay.w)).all()
        self.host = inp.walk_buffer(lay)
        self.buf = dev(self.host)
        self.ff = SimpleNamespace(view=self.buf[lay.off:], pitch=lay.pitch)   # what Walk.fresh makes its levels on
        self.fm_host = inp.hood_mask(lay.w, lay.h)
        self.fm = dev(self.fm_host)
        self.mvps, self.Ms = views(self.sc.rp, S), warps(lay.w, lay.h, WN)
        self.refs = {}
        self.tone = "shift"   # the walking level's tone map (as created: the default)

    def set_lens(self, lv, lens):
        if lens == "none":
            lv.set_distortion(None, None)
        elif lens == "barrel":
            lv.set_distortion(self.K, inp.BARREL)
        else:
            lv.set_distortion_fisheye(self.K, self.Kr, inp.FISHEYE)

    def set_format(self, lv, frame):
        """The frame setter of a reading, without its tone map."""
        factor, fmt, _ = inp.frame_spec(frame)
        if frame == "off":
            lv.set_frame_reduction(1, cnp.GRAY, 0)
        elif factor == 1:
            lv.set_frame_format(fmt, self.lay.pitch)
        else:
            lv.set_frame_reduction(factor, fmt, self.lay.pitch)

    def set_tone(self, lv, tone):
        lv.set_tone_map(None if tone == "shift" else tnp.capi_tone(capi, inp.TONES[tone]))

    def move_frame(self, lv, kind, lens, src, dst, i):
        """The walking level from frame src to frame dst (move i), compared wherever it passes through a deep reading."""
        fs, fd = inp.frame_spec(src), inp.frame_spec(dst)
        if fd[2] is None:                               # to a non-deep value: the tone map stays set, ignored
            self.set_format(lv, dst)
        elif fs[2] is not None and fs[0] == fd[0]:      # between two deep values of one factor: the tone map alone
            self.set_tone(lv, fd[2])
            self.tone = fd[2]
        elif inp.call_order(i, self.origin) == "tone-first":
            self.set_tone(lv, fd[2])
            self.tone = fd[2]
            if fs[2] is not None:                       # (from the deep value of the other factor: not ignored)
                self.check(lv, (kind, lens, inp.deep_name(fs[0], self.tone)), f"move {i}: {src} under the tone map of {dst}")
            self.set_format(lv, dst)
        else:
            self.set_format(lv, dst)
            self.check(lv, (kind, lens, inp.deep_name(fd[0], self.tone)), f"move {i}: the format of {dst} under the tone map before")
            self.set_tone(lv, fd[2])
            self.tone = fd[2]

    def put(self, lv, state):
        """A level as created straight into the state: frame (and tone map), lens, kind."""
        kind, lens, frame = state
        if frame != "off":
            self.set_format(lv, frame)
        tone = inp.frame_spec(frame)[2]
        if tone not in (None, "shift"):
            self.set_tone(lv, tone)
        if lens != "none":
            self.set_lens(lv, lens)
        self.set_kind(lv, "plain", kind)

    def reference(self, state):
        if state not in self.refs:
            with self.fresh() as ref:
                self.put(ref, state)
                self.refs[state] = self.snapshot(ref, state)
                self.tie(ref, state)
        return self.refs[state]

    def tie(self, ref, state):
        """The reference against the twins: its warps are those of the twin's frame and mask, uploaded as a plain grey frame,
        and its winner and ratings the standalone search's on them."""
        kind, lens, frame = state
        lay = self.lay
        raw_mask = None if kind == "plain" else self.fm_host
        grey, mask = inp.grey_of(self.host, lay.w, lay.h, lay.pitch, lay.off, (lens, frame), raw_mask, K=self.K)
        win = ref.run(self.mvps, self.Ms)
        rs, ws, t = ref.outputs()
        cw, ct, cws, cwm = rest_of_chain(self.ctx, self.sc, dev(grey), kind, self.K, None, None if kind == "plain" else dev(mask),
                                         self.mvps, self.Ms, rs)
        assert (cws == ws).all(), f"{state}: the level's warps are not those of the twin's frame"
        if kind == "masked":
            assert (ref.masks()[0] == cwm).all(), f"{state}: the level's warp masks are not those of the twin's mask"
        if kind == "covered":
            assert (ref.coverage()[1] == cwm).all(), f"{state}: the level's warp masks are not those of the twin's mask"
        assert cw == win and (bits(ct) == bits(t)).all(), (state, cw, win)


def first_at(edges, start, deep):
    """The first move from number `start` on that ends in a deep (or a non-deep) frame."""
    return next(i for i, (_, dst) in enumerate(edges) if i >= start and inp.is_deep(dst[1]) == deep)


@pytest.mark.parametrize("layout", list(inp.LAYOUTS))
@pytest.mark.parametrize("kind", KINDS)
def test_one_level_walks_every_move_between_its_intakes(nmi, kind, layout):
    lay = inp.LAYOUTS[layout]
    axes = (inp.LENSES, inp.FRAME_NAMES)
    edges = wp.check_circuit(wp.euler_circuit(START, axes), START, axes)
    assert len(edges) == 270
    bad_tone = capi.ToneMap(mode=capi.TONE_WINDOW, bits=16, lo=700, hi=700)
    refusals = {first_at(edges, 30, True): "a bad tone map in a deep state", first_at(edges, 75, False): "a bad tone map in a non-deep state",
                120: "an odd pitch for GRAY16", 165: "a Bayer pitch below the width", 210: "a skewed K for the fisheye setter"}
    assert len(refusals) == 5
    with nmi.NmiContext(lay.w, lay.h) as ctx:
        wk = IntakeWalk(nmi, ctx, lay, origin=KINDS.index(kind) % 2)
        skew = wk.K.copy()
        skew[0, 1] = 0.5
        with wk.fresh() as lv:
            wk.check(lv, OFF, "as created")
            wk.set_format(lv, START[1])                                         # off -> the circuit's first state
            wk.check(lv, ("plain",) + START, "towards the start")
            wk.set_kind(lv, "plain", kind)
            wk.check(lv, (kind,) + START, "at the start")
            for i, (src, dst) in enumerate(edges):
                if src[0] != dst[0]:
                    wk.set_lens(lv, dst[0])
                else:
                    wk.move_frame(lv, kind, src[0], src[1], dst[1], i)
                wk.check(lv, (kind,) + dst, f"move {i} {src} -> {dst}")
                what = refusals.get(i)
                if what:
                    with pytest.raises(capi.NmiError):
                        if "tone map" in what:
                            lv.set_tone_map(bad_tone)
                        elif "GRAY16" in what:
                            lv.set_frame_format(capi.FRAME_GRAY16, lay.pitch + 1)
                        elif "Bayer" in what:
                            lv.set_frame_format(capi.FRAME_BAYER_GRBG, lay.w - 1)
                        else:
                            lv.set_distortion_fisheye(skew, wk.Kr, inp.FISHEYE)
                    wk.check(lv, (kind,) + dst, f"after {what}, refused in {dst}")
            wk.set_kind(lv, kind, "plain")                                      # ... and back to off; the tone map stays set
            wk.check(lv, ("plain",) + START, "kind off")
            wk.set_format(lv, "off")
            wk.check(lv, OFF, "everything off again")
        assert {(kind,) + s for s in inp.STATES} <= set(wk.refs)


@pytest.mark.parametrize("layout", list(inp.LAYOUTS))
@pytest.mark.parametrize("frame", ["grbg", "deep-eq", "deep-pct-f2"])
def test_kinds_and_lenses_under_two_node_and_deep_intakes(nmi, frame, layout):
    lay = inp.LAYOUTS[layout]
    axes = (KINDS, inp.LENSES)
    start = ("plain", "none")
    edges = wp.check_circuit(wp.euler_circuit(start, axes), start, axes)
    assert len(edges) == 36
    at_masked = next(i for i, (_, dst) in enumerate(edges) if i >= 12 and dst[0] == "masked")
    with nmi.NmiContext(lay.w, lay.h) as ctx:
        wk = IntakeWalk(nmi, ctx, lay)
        with wk.fresh() as lv:
            wk.put(lv, start + (frame,))
            wk.check(lv, start + (frame,), "at the start")
            for i, (src, dst) in enumerate(edges):
                if src[0] != dst[0]:
                    wk.set_kind(lv, src[0], dst[0])
                else:
                    wk.set_lens(lv, dst[1])
                wk.check(lv, dst + (frame,), f"move {i} {src} -> {dst}")
                if i == at_masked:
                    with pytest.raises(capi.NmiError):
                        lv.set_coverage(True, wk.fm)
                    wk.check(lv, dst + (frame,), f"after set_coverage on a masked level, refused in {dst}")
            wk.set_format(lv, "off")
            wk.check(lv, OFF, "frame setting off")
        assert {s + (frame,) for s in wp.states(axes)} <= set(wk.refs)
