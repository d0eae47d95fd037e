"""GPU test (-m gpu) of every transition between a level's settings (nmi_level_set_masks / _set_coverage / _set_distortion /
_set_frame_format / _set_frame_reduction).

A state is (kind, lens, frame): kind plain / masked / covered, lens none / barrel, frame gray / format / reduced -- 18 states.
A move changes one axis through the public setter (masked <-> covered is two calls, off then on), so every state has 5 moves:
90 directed moves.  ONE level walks a fixed Euler circuit over all 90; after each move it is run once and compared byte for byte
-- winner, renders, warps, ratings, masks and counts or coverage masks and counts -- with a fresh level that was put straight
into that state and run on the same inputs.  What this pins is the lifetime of the buffers a setting brings with it: one freed
while a graph still reads it, or a stale one read after a switch, shows as a difference (or a fault) at the move that did it.

The frame axis on one buffer: the level is created on a full-size (factor 2) RGB buffer with a padded pitch.  "reduced" is
set_frame_reduction(2, RGB, pitch) on it; "format" is set_frame_format(RGB, pitch), which reads its first H rows of W pixels;
"gray" is set_frame_format(GRAY, pitch) over the same bytes -- a pitch that is not the dense one, so it is a setting like the
other two, not "off".  "Off" -- (1, GRAY, 0), no lens, plain: the level as created -- is the walk's start and end: the level goes
from it to the circuit's first state one setter at a time, and back to it after the circuit, each step compared too."""
import numpy as np
import pytest

from helpers import color_np as cnp
from helpers import undistort_np as unp
from helpers.walk_plan import euler_circuit, neighbours
from orbslam2_nmi_amd import capi
from test_color_level import enable, lens_K
from test_covered_level import CoveredScene
from test_masked_level import dev, hood_mask, views, warps
from test_reduce_level import FullFrame, level

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

KINDS, LENSES, FRAMES = ("plain", "masked", "covered"), ("none", "barrel"), ("gray", "format", "reduced")
AXES = (KINDS, LENSES, FRAMES)
STATES = [(k, l, f) for k in KINDS for l in LENSES for f in FRAMES]
OFF = ("plain", "none", "off")
START = ("covered", "barrel", "reduced")
FACTOR = 2


@pytest.fixture(scope="module")
def nmi():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    import orbslam2_nmi_amd as m
    m.load_library()
    return m


class Walk:
    """The inputs all levels of one parametrisation share, the setters by axis, and the cached references."""

    def __init__(self, nmi, ctx, w, h, mesh, pad, S, Wn):
        self.nmi, self.ctx, self.S, self.Wn = nmi, ctx, S, Wn
        self.sc = CoveredScene(nmi, ctx, w, h, mesh)
        self.K, self.dist = lens_K(self.sc.rp), unp.FAMILIES["barrel"]
        self.ff = FullFrame(self.sc, FACTOR, cnp.RGB, FACTOR * w * 3 + pad, 0)
        self.fm = dev(hood_mask(w, h))
        self.mvps, self.Ms = views(self.sc.rp, S), warps(w, h, Wn)
        self.refs = {}

    def fresh(self):
        return level(self.nmi, self.sc, self.ff, self.S, self.Wn)

    def set_kind(self, lv, was, kind):
        if was == "masked":
            lv.set_masks(False)
        if was == "covered":
            lv.set_coverage(False)
        enable(lv, kind, self.fm)

    def set_lens(self, lv, lens):
        if lens == "none":
            lv.set_distortion(None, None)
        else:
            lv.set_distortion(self.K, self.dist)

    def set_frame(self, lv, frame):
        if frame == "off":
            lv.set_frame_reduction(1, cnp.GRAY, 0)
        elif frame == "reduced":
            lv.set_frame_reduction(FACTOR, cnp.RGB, self.ff.pitch)
        else:
            lv.set_frame_format(cnp.GRAY if frame == "gray" else cnp.RGB, self.ff.pitch)

    def move(self, lv, src, dst):
        assert sum(a != b for a, b in zip(src, dst)) == 1, (src, dst)
        if src[0] != dst[0]:
            self.set_kind(lv, src[0], dst[0])
        elif src[1] != dst[1]:
            self.set_lens(lv, dst[1])
        else:
            self.set_frame(lv, dst[2])

    def snapshot(self, lv, state):
        """One run -> everything the level hands out in that state, as byte arrays."""
        win = lv.run(self.mvps, self.Ms)
        out = [np.array(win[0], np.int64), np.array(win[1], np.float32)] + list(lv.outputs())
        if state[0] == "masked":
            out += list(lv.masks())
        if state[0] == "covered":
            out += list(lv.coverage())
        return [np.ascontiguousarray(a).reshape(-1).view(np.uint8) for a in out]

    def put(self, lv, state):
        """A level as created straight into the state: frame, lens, kind."""
        if state[2] != "off":
            self.set_frame(lv, state[2])
        if state[1] != "none":
            self.set_lens(lv, state[1])
        enable(lv, state[0], self.fm)

    def reference(self, state):
        """A fresh level put straight into the state and run once; made once per state."""
        if state not in self.refs:
            with self.fresh() as ref:
                self.put(ref, state)
                self.refs[state] = self.snapshot(ref, state)
        return self.refs[state]

    def check(self, lv, state, what):
        got, want = self.snapshot(lv, state), self.reference(state)
        names = ["winner", "score", "renders", "warps", "ratings"] + {"plain": [], "masked": ["warp masks", "counts"],
                                                                      "covered": ["render masks", "warp masks", "counts"]}[state[0]]
        assert len(got) == len(want) == len(names)
        for name, a, b in zip(names, got, want):
            assert a.size == b.size and (a == b).all(), f"{what}: {name} differ from a fresh level in {state}"


# 160x120: rows of whole 16-byte chunks (the fused front kernels, 16-byte loads of the padded rows); 100x75: neither (the byte
# paths, the warp on the forked branch, an odd pitch)
SHAPES = [(160, 120, 16), (100, 75, 5)]


@pytest.mark.parametrize("mesh", [False, True], ids=["cloud", "mesh"])
@pytest.mark.parametrize("shape", SHAPES, ids=["160x120", "100x75"])
def test_one_level_walks_every_move_between_its_settings(nmi, shape, mesh):
    w, h, pad = shape
    circuit = euler_circuit(START, AXES)
    edges = list(zip(circuit[:-1], circuit[1:]))
    assert len(edges) == 90 and len(set(edges)) == 90 and set(circuit) == set(STATES) and circuit[0] == circuit[-1] == START
    assert all(dst in neighbours(src, AXES) for src, dst in edges)
    # rejected calls at fixed points of the walk: after these moves (the third one at the first masked state from move 60 on)
    at_masked = next(i for i, (_, dst) in enumerate(edges) if i >= 60 and dst[0] == "masked")
    with nmi.NmiContext(w, h) as ctx:
        wk = Walk(nmi, ctx, w, h, mesh, pad, 3, 3)
        skew = wk.K.copy()
        skew[0, 1] = 0.5
        with wk.fresh() as lv:
            wk.check(lv, OFF, "as created")
            wk.set_frame(lv, START[2])                                          # off -> the circuit's first state
            wk.check(lv, ("plain", "none", START[2]), "towards the start")
            wk.set_lens(lv, START[1])
            wk.check(lv, ("plain",) + START[1:], "towards the start")
            wk.set_kind(lv, "plain", START[0])
            wk.check(lv, START, "at the start")
            for i, (src, dst) in enumerate(edges):
                wk.move(lv, src, dst)
                wk.check(lv, dst, f"move {i} {src} -> {dst}")
                rejected = None
                if i == 20:
                    with pytest.raises(capi.NmiError):
                        lv.set_frame_reduction(5, cnp.RGB, wk.ff.pitch)
                    rejected = "a bad factor"
                if i == 40:
                    with pytest.raises(capi.NmiError):
                        lv.set_distortion(skew, wk.dist)
                    rejected = "a bad K"
                if i == at_masked:
                    with pytest.raises(capi.NmiError):
                        lv.set_coverage(True, wk.fm)
                    rejected = "set_coverage on a masked level"
                if rejected:
                    wk.check(lv, dst, f"after {rejected}, refused in {dst}")
            wk.set_frame(lv, "off")                                             # ... and back to off
            wk.check(lv, START[:2] + ("off",), "frame setting off")
            wk.set_lens(lv, "none")
            wk.check(lv, (START[0], "none", "off"), "lens off")
            wk.set_kind(lv, START[0], "plain")
            wk.check(lv, OFF, "everything off again")
        assert set(STATES) <= set(wk.refs)
