"""The plan of the intake walks (tests/test_intake_level_walk.py, tests/test_intake_stream_walk.py), checked without a GPU.

The walks compare a level or a stream that moves between intake settings with one put straight into each setting.  That only
bites if a stale frame -- the frame of the state before, or of any other state -- cannot pass for the right one.  So, per
layout and from the CPU twins alone (tests/helpers/intake_np.py): the 27 grey frames of (lens, frame) on the walk's buffer are
pairwise different and each holds at least 32 distinct grey values; so do the deep readings a walk passes through between two
setter calls; and the lens states' masks are neither empty nor full.  Also here: the properties of the circuits the walks
follow -- every state visited, every directed move exactly once, first state == last state."""
import itertools

import numpy as np
import pytest

from helpers import intake_np as inp
from helpers import walk_plan as wp

KINDS = ("plain", "masked", "covered")


@pytest.fixture(scope="module", params=list(inp.LAYOUTS))
def frames(request):
    """layout, {(lens, frame): (grey, mask)} for the 27 states and for every deep reading a walk can pass through."""
    lay = inp.LAYOUTS[request.param]
    buf = inp.walk_buffer(lay)
    assert buf.size == lay.nbytes
    passing = [inp.deep_name(f, t) for f in (1, 2) for t in inp.TONES]
    names = list(inp.FRAME_NAMES) + [n for n in passing if n not in inp.FRAMES]
    return lay, {(lens, fr): inp.grey_of(buf, lay.w, lay.h, lay.pitch, lay.off, (lens, fr)) for lens in inp.LENSES for fr in names}


def test_layouts_reach_the_paths_they_are_for():
    a, b = inp.LAYOUTS["A"], inp.LAYOUTS["B"]
    assert (a.w, a.h, a.pitch, a.off) == (64, 48, 2 * 64 * 3 + 16, 0) and a.w % 16 == 0 and a.pitch % 16 == 0
    assert (b.w, b.h, b.pitch, b.off) == (50, 38, 2 * 50 * 3 + 6, 2)
    assert b.pitch % 2 == 0 and b.pitch % 4 != 0 and b.off % 2 == 0 and b.w % 4 != 0 and b.w >= 32
    for lay in (a, b):   # every reading fits a row: 2W pixels of up to 3 bytes
        assert lay.pitch >= 2 * lay.w * 3


def test_the_27_frames_are_pairwise_different_and_rich(frames):
    lay, got = frames
    states = [(lens, fr) for lens in inp.LENSES for fr in inp.FRAME_NAMES]
    assert len(states) == 27 and states == inp.STATES
    for s in states:
        grey = got[s][0]
        assert grey.shape == (lay.h, lay.w) and grey.dtype == np.uint8
        assert np.unique(grey).size >= 32, (lay.name, s, np.unique(grey).size)
    for a, b in itertools.combinations(states, 2):
        differ = int((got[a][0] != got[b][0]).sum())
        assert differ > 0, (lay.name, a, b)


def test_the_readings_a_walk_passes_through_differ_from_their_neighbours(frames):
    """A move into a deep state is two calls; between them the level is in (format, the tone map before).  Those frames are
    checked too, so they must differ from every named deep frame under the same lens, and from each other."""
    lay, got = frames
    for lens in inp.LENSES:
        deep = [fr for (l, fr) in got if l == lens and inp.is_deep(fr)]
        assert len(deep) == 8
        for a, b in itertools.combinations(deep, 2):
            assert (got[(lens, a)][0] != got[(lens, b)][0]).any(), (lay.name, lens, a, b)
        for fr in deep:
            assert np.unique(got[(lens, fr)][0]).size >= 32, (lay.name, lens, fr)


def test_lens_masks_differ(frames):
    """The fisheye states' mask has an invalid border; the barrel lens reads inside the frame everywhere, so its mask shows only
    under a frame mask, which it moves."""
    lay, got = frames
    none, barrel, fisheye = (got[(lens, "gray")][1] for lens in inp.LENSES)
    assert none.all() and barrel.all()
    assert 0 < int(fisheye.sum()) < lay.w * lay.h
    hood = inp.hood_mask(lay.w, lay.h)
    buf = inp.walk_buffer(lay)
    masks = [inp.grey_of(buf, lay.w, lay.h, lay.pitch, lay.off, (lens, "gray"), hood)[1] for lens in inp.LENSES]
    assert (masks[0] == hood).all()
    for a, b in itertools.combinations(masks, 2):
        assert (a != b).any()
    assert all(0 < int(m.sum()) < lay.w * lay.h for m in masks)


def test_equalize_is_not_a_shift(frames):
    """Uniform 16-bit noise would make EQUALIZE look like SHIFT; the buffer is skewed so that it does not, by a wide margin."""
    lay, got = frames
    eq, shift = got[("none", "deep-eq")][0].astype(int), got[("none", inp.deep_name(1, "shift"))][0].astype(int)
    assert np.abs(eq - shift).mean() > 16


def test_walk_f_circuit():
    axes = (inp.LENSES, inp.FRAME_NAMES)
    start = (inp.LENSES[0], inp.FRAME_NAMES[0])
    edges = wp.check_circuit(wp.euler_circuit(start, axes), start, axes)
    assert len(edges) == 270 and len(set(edges)) == 270
    assert all(len(wp.neighbours(s, axes)) == 10 for s in wp.states(axes))
    assert sum(a[0] != b[0] for a, b in edges) == 27 * 2 and sum(a[1] != b[1] for a, b in edges) == 27 * 8
    # A move into a deep value is two calls, in an order that goes by the move's number.  The walks number their moves from 0
    # or from 1 (inp.call_order); between the two, every such move is made in both orders.
    into = [i for i, (a, b) in enumerate(edges) if a[1] != b[1] and inp.is_deep(b[1]) and not inp.is_deep(a[1])]
    assert len(into) == 3 * 6 * 3
    for i in into:
        assert {inp.call_order(i, 0), inp.call_order(i, 1)} == {"tone-first", "frame-first"}
    for origin in (0, 1):   # ... and either numbering alone walks both orders, though not under every lens
        assert {inp.call_order(i, origin) for i in into} == {"tone-first", "frame-first"}


def test_walk_k_circuit():
    axes = (KINDS, inp.LENSES)
    start = ("plain", "none")
    edges = wp.check_circuit(wp.euler_circuit(start, axes), start, axes)
    assert len(edges) == 36 and len(set(edges)) == 36


def test_the_existing_walks_circuit_is_unchanged():
    """tests/test_level_settings_walk.py: 18 states, 90 moves, from the helper the walks now share."""
    axes = (KINDS, ("none", "barrel"), ("gray", "format", "reduced"))
    start = ("covered", "barrel", "reduced")
    circuit = wp.euler_circuit(start, axes)
    edges = wp.check_circuit(circuit, start, axes)
    assert len(edges) == 90
    assert circuit[:4] == [start, ("plain", "barrel", "reduced"), ("masked", "barrel", "reduced"), ("plain", "barrel", "reduced")]
