"""CPU tests of the launch-geometry mirror (tests/helpers/intake_geometry.py) and of the premises of the GPU tests that choose
their sizes by it (tests/helpers/seam_cases.py; tests/test_packed_seams.py, tests/test_valid_seams.py and the second-trip cases of
tests/test_clahe_tables.py): the mirror's constants are the kernels' own, read out of the .hip sources, and every size reaches
the block column, tail, store path or loop trip it is listed for.  A retuned kernel fails here instead of hollowing those tests
out."""
import os
import re

import numpy as np
import pytest

from helpers import clahe_np as cnp
from helpers import intake_geometry as geo
from helpers import packed_np as pnp
from helpers import seam_cases as cases
from helpers import valid_cases
from helpers import valid_np as vnp

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "orbslam2_nmi_amd", "csrc")


def source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def constant(text, name):
    found = re.findall(r"constexpr\s+int\s+" + name + r"\s*=\s*(\d+)\s*;", text)
    assert len(found) == 1, (name, found)
    return int(found[0])


# --- the constants ------------------------------------------------------------------------------------------------------------------

def test_the_unpack_constants_are_the_kernels():
    text = source("nmi_unpack.hip")
    assert constant(text, "kUnpackLanes") == geo.kUnpackLanes
    # a lane's run of 8 pixels, and the block row of kUnpackLanes lanes, in both kernels and the launcher
    assert len(re.findall(r"const int run = blockIdx\.x \* kUnpackLanes \+ \(int\)threadIdx\.x;", text)) == 2
    assert len(re.findall(r"const int x0 = run \* (\d+);", text)) == 2
    assert {int(n) for n in re.findall(r"const int x0 = run \* (\d+);", text)} == {geo.kUnpackRun}
    runs = re.findall(r"const int runs = \(width \+ (\d+)\) / (\d+);", text)
    assert runs == [(str(geo.kUnpackRun - 1), str(geo.kUnpackRun))]
    assert re.search(r"grid\(\(runs \+ kUnpackLanes - 1\) / kUnpackLanes, \(height \+ 3\) / 4\), block\(kUnpackLanes, 4\)", text)
    vec = re.search(r"const int vec = \(base % (\d+)\) == 0 && \(width % (\d+)\) == 0 \? 2 : \(base % (\d+)\) == 0 && \(width % (\d+)\) == 0 \? 1 : 0;", text)
    assert vec and [int(g) for g in vec.groups()] == [16, 8, 8, 4]


GRID = r"const int quads = \(width \+ (\d+)\) / (\d+);\s*const dim3 grid\(\(quads \+ (\d+)\) / (\d+), \(height \+ 3\) / 4\), block\((\d+), 4\);"


@pytest.mark.parametrize("name,own", [("nmi_tone.hip", "nmi_gray16"), ("nmi_clahe.hip", "nmi_clahe_gray16")])
def test_the_conversion_constants_are_the_kernels(name, own):
    text = source(name)
    x0 = re.findall(r"const int x0 = \(blockIdx\.x \* (\d+) \+ \(int\)threadIdx\.x\) \* (\d+);", text)
    assert x0 == [(str(geo.kBlockRowLanes), str(geo.kQuad))], x0            # (one kernel template, plain and masked)
    # the launch grid: defined once, in nmi_tone.h's quad_launch; each file launches both instantiations by it and has none of its own
    grids = re.findall(GRID, source("nmi_tone.h"))
    want = tuple(str(v) for v in (geo.kQuad - 1, geo.kQuad, geo.kBlockRowLanes - 1, geo.kBlockRowLanes, geo.kBlockRowLanes))
    assert grids == [want], grids
    assert len(re.findall(r"const QuadLaunch q = quad_launch\(", text)) == 1
    launches = re.findall(own + r"_kernel<F, (true|false)>\), q\.grid, q\.block,", text)
    assert sorted(launches) == ["false", "true"], launches
    assert not re.search(r"int quads\b|dim3 grid\(|block\(\d+|<<<", text), "a grid of the file's own"


def test_the_histogram_constants_are_the_kernels():
    tone, clahe = source("nmi_tone.hip"), source("nmi_clahe.hip")
    for name in ("kHistThreads", "kHistRun", "kHistRunsPerLane", "kHistMaxWorkgroups"):
        assert constant(tone, name) == getattr(geo, name), name
    for name in ("kHistThreads", "kHistPerLane", "kHistMaxWorkgroups"):
        assert constant(clahe, name) == getattr(geo, name), name
    assert re.search(r"constexpr int kHistChunk = kHistThreads \* kHistPerLane;", clahe)
    assert geo.kHistChunk == geo.kHistThreads * geo.kHistPerLane == 4096
    # the loops the trips are counted for
    assert re.search(r"const uint32_t chunk = gridDim\.x \* \(uint32_t\)\(kHistThreads \* kHistRunsPerLane\);", tone)
    assert re.search(r"for \(uint32_t first = 0; first < items; first \+= chunk\)", tone)
    assert re.search(r"first = \(uint64_t\)blockIdx\.x \* kHistChunk; first < n; first \+= \(uint64_t\)gridDim\.x \* kHistChunk", clahe)
    # the ranged kernels are instantiations of these templates, not units of their own with constants of their own
    for twin in ("nmi_tone_valid.hip", "nmi_clahe_valid.hip"):
        assert not os.path.exists(os.path.join(CSRC, twin)), twin
    assert len(re.findall(r"template <bool Ranged, class\.\.\. Range>\s*__global__ __launch_bounds__\(kHistThreads\) void nmi_tone_hist_kernel\(", tone)) == 1
    assert len(re.findall(r"template <bool Ranged, class\.\.\. Range>\s*__global__ __launch_bounds__\(kHistThreads\) void nmi_clahe_hist_kernel\(", clahe)) == 1


@pytest.mark.parametrize("tiles,size", [(8, 2101), (8, 2011), (8, 2104), (8, 2012), (3, 264), (2, 8), (8, 8), (8, 9), (3, 783), (8, 64),
                                        (8, 70), (1, 37)])
def test_the_tile_edges_are_the_models_tiles(tiles, size):
    """The host's closed form for the edges == where clahe_np's tile rule changes its value."""
    edges = geo.clahe_edges(tiles, size)
    t = cnp.tile_of(size, tiles)
    assert edges[0] == 0 and edges[-1] == size and len(edges) == tiles + 1
    for i in range(tiles):
        assert (t[edges[i]:edges[i + 1]] == i).all() and edges[i + 1] > edges[i]


def test_the_mirror_on_known_sizes():
    assert [geo.unpack_runs(w) for w in (1, 8, 9, 512, 513)] == [1, 1, 2, 64, 65]
    assert [geo.unpack_blocks(w) for w in (1, 512, 513, 1024, 1025)] == [1, 1, 2, 2, 3]
    assert [geo.unpack_tail(w) for w in (1, 7, 8, 9, 516, 520)] == [1, 7, 8, 1, 4, 8]
    assert [geo.convert_blocks(w) for w in (1, 256, 257, 261, 264, 513)] == [1, 1, 2, 2, 2, 3]
    assert [geo.convert_tail(w) for w in (261, 264, 37)] == [1, 4, 1]
    assert geo.tone_hist(2896, 1450) == (362 * 1450, 1024, 2)              # test_a_frame_of_more_than_one_histogram_chunk
    assert geo.tone_hist(160, 96)[2] == 1 and geo.tone_hist(1, 1) == (1, 1, 1)
    # the nearest misses: 256 x 130 in 2 x 1 tiles is 5 chunks over 5 workgroups; a 65,536-pixel tile is 16 x 4096, one trip
    assert geo.clahe_per_tile(2, 1, 256, 130) == 5 and (geo.clahe_trips(2, 1, 256, 130) == 1).all()
    assert geo.clahe_per_tile(8, 8, 1 << 19, 8) == 16 and (geo.clahe_tile_pixels(8, 8, 1 << 19, 8) == 65536).all()
    assert (geo.clahe_trips(8, 8, 1 << 19, 8) == 1).all()


# --- nmi_unpack_frame's cases -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", pnp.LAYOUTS)
def test_the_unpack_widths_reach_every_tail_and_three_block_columns(fmt):
    widths = cases.UNPACK_WIDTHS[fmt]
    assert all(pnp.row_bytes(fmt, w) > 0 for w in widths)
    assert {geo.unpack_tail(w) for w in widths} == cases.UNPACK_TAILS[fmt]
    # every tail also in a last run that lies in block column 1 or 2 (lane 64 and above: the run * NB byte offset)
    far = [w for w in widths if geo.unpack_blocks(w) >= 2]
    assert {geo.unpack_tail(w) for w in far} >= cases.UNPACK_TAILS[fmt] - ({3, 5} if fmt == pnp.GRAY16_BE else set())
    assert max(geo.unpack_blocks(w) for w in widths) == 3 and min(geo.unpack_blocks(w) for w in widths) == 1
    if pnp.GROUP[fmt] == (2, 3):    # the partial runs of 3 and 9 source bytes
        assert {geo.unpack_tail_bytes(w, 2, 3) for w in widths} >= {3, 6, 9}
    # the dense store paths by the width alone (an allocator's base), and the factor-3 source across the seam
    assert {geo.unpack_vec(0, w) for w in widths} == ({0, 1, 2} if fmt != pnp.MONO10P and fmt != pnp.RAW10 else {1, 2})
    w3 = 3 * cases.UNPACK_FACTOR3[0]
    assert pnp.row_bytes(fmt, w3) > 0 and geo.unpack_blocks(w3) == 2


@pytest.mark.parametrize("fmt", pnp.FORMATS)
def test_every_store_path_is_chosen_by_the_base(fmt):
    """520 wide: vec 2, 1 and 0 by the base alone; 516: 1 and 0; 518 (not the 10-bit layouts): 0 whatever the base."""
    widths = cases.out_widths(fmt)
    assert widths == ((520, 516) if pnp.GROUP[fmt][0] == 4 else (520, 516, 518))
    by_width = {w: [geo.unpack_vec(b, w) for b in cases.OUT_BASES] for w in widths}
    assert by_width[520] == [2, 0, 1, 0] and by_width[516] == [1, 0, 1, 0]
    assert fmt in (pnp.MONO10P, pnp.RAW10) or by_width[518] == [0, 0, 0, 0]
    assert all(geo.unpack_blocks(w) == 2 for w in widths)
    # the halves of the decision an aligned base never shows: base % 16 and base % 8 false on a width that allows the store
    assert geo.unpack_vec(8, 520) == 1 and geo.unpack_vec(2, 520) == 0 and geo.unpack_vec(2, 516) == 0


def test_the_mosaic_sizes_put_windows_on_both_sides_of_the_seam():
    seam = geo.kUnpackLanes * geo.kUnpackRun
    assert seam == 512
    for w, h in cases.BAYER_SIZES:
        assert geo.unpack_blocks(w) >= 2 and h >= 2
        runs = geo.unpack_runs(w)
        # run 63's window reads site 512 (row[8]), run 64's site 511 (row[-1]); which of them are interior windows
        interior = [r for r in range(runs) if 8 * r >= 1 and 8 * r + 8 < w and h >= 3]
        if h >= 3:
            assert 63 in interior
        assert (64 in interior) == (h >= 3 and 520 < w)
    assert any(geo.unpack_blocks(w) == 3 for w, _ in cases.BAYER_SIZES)
    assert {geo.unpack_tail(w) for w, _ in cases.BAYER_SIZES} == {1, 2, 7, 8}
    assert any(h == 2 for _, h in cases.BAYER_SIZES)                        # every row a reflected one
    for pattern, fmt in pnp.BAYER16.items():                                # a flat mosaic is white
        assert (pnp.bayer16_gray(np.full((3, 10), 65535, np.uint16), fmt) == 65535).all(), pattern
    assert geo.unpack_blocks(cases.CHAIN_SIZE[0]) == 2 and all(pnp.row_bytes(f, cases.CHAIN_SIZE[0]) > 0 for f in pnp.FORMATS)


# --- the valid-range conversions' cases ---------------------------------------------------------------------------------------------

def test_the_valid_sizes_cross_the_block_seam():
    assert cases.SEAM == geo.kQuad * geo.kBlockRowLanes == 256
    (wa, ha), (wb, hb) = cases.VALID_SIZES
    assert geo.convert_blocks(wa) == geo.convert_blocks(wb) == 2
    assert geo.convert_tail(wa) == 4 and wa % 4 == 0                        # vector stores
    assert geo.convert_tail(wb) == 1                                        # the last quad partial: byte stores
    assert min(ha, hb) >= 8                                                 # the 8 x 8 grid: no empty tile row
    for w, h in cases.VALID_SIZES:
        for f in valid_cases.FACTORS:
            for tx, ty in ((1, 1), (3, 2), (8, 8)):
                assert (geo.clahe_tile_pixels(tx, ty, f * w, f * h) > 0).all()
    # the plain kernels' additions: tests/test_tone_reduce.py and tests/test_clahe_frame.py
    assert geo.convert_blocks(261) == geo.convert_blocks(264) == 2


@pytest.mark.parametrize("size", cases.VALID_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", cases.VALID_FRAMES)
def test_the_valid_frames_have_invalid_pixels_on_both_sides_of_the_seam(name, size):
    w, h = size
    for f in valid_cases.FACTORS:
        px, rng, bits = cases.valid_frame(name, w, h, f)
        assert px.shape == (f * h, f * w) and vnp.is_on(rng)
        m = vnp.mask(px, f, rng)
        assert (m[:, :cases.SEAM] == 0).any() and (m[:, cases.SEAM:] == 0).any(), (name, f)
        assert (m == 1).any(), (name, f)
        assert {geo.convert_block_of(x) for x in np.argwhere(m == 0)[:, 1]} == {0, 1}
        # the range is in the statistics: the ranged histogram is not the plain one
        assert (vnp.histogram(px, bits, rng) != vnp.histogram(px, bits, vnp.OFF)).any()


@pytest.mark.parametrize("size", cases.VALID_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_seam_pixels_is_three_zeros_of_the_mask(size):
    w, h = size
    spots = None
    for f in valid_cases.FACTORS:
        px, rng, bits, zeros = vnp.seam_pixels(f * w, f * h, f, cases.seam_columns(w), seed=1)
        assert (px == cases.valid_frame("seam_pixels", w, h, f)[0]).all()
        assert int((~vnp.valid(px, rng)).sum()) == 3
        m = vnp.mask(px, f, rng)
        assert sorted(map(tuple, np.argwhere(m == 0)[:, ::-1].tolist())) == sorted(zeros)
        assert [x for x, _ in zeros] == [255, 256, w - 1] and len({y for _, y in zeros}) == 3
        bad = np.argwhere(~vnp.valid(px, rng))
        corners = {(int(y) % f, int(x) % f) for y, x in bad}
        assert len(corners) == min(3, f * f)                                # three different corners of their blocks
        assert spots is None or spots == zeros                              # the same output pixels at every factor
        spots = zeros


# --- the second trips ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("run", list(cases.SECOND_TRIP_RUNS))
def test_the_tone_histogram_takes_a_second_chunk(run):
    w, h, f = cases.SECOND_TRIP_RUNS[run]
    ws, hs = f * w, f * h
    items, workgroups, trips = geo.tone_hist(ws, hs)
    assert items == 263 * hs > 1024 * 512 and workgroups == geo.kHistMaxWorkgroups and trips == 2
    trip = geo.tone_hist_trip_map(ws, hs)
    assert set(np.unique(trip)) == {0, 1}
    late_rows = np.flatnonzero((trip == 1).any(axis=1))
    assert late_rows[-1] == hs - 1 and (np.diff(late_rows) == 1).all()      # the last rows of the frame ...
    assert 0 < (trip[late_rows[0]] == 1).sum() < ws                         # ... from the middle of one
    assert (trip == 1).sum() < 512 * 8 * workgroups                         # a ragged second trip: some workgroups have nothing
    assert geo.convert_blocks(w) >= (3 if f == 4 else 2)


@pytest.mark.parametrize("run", list(cases.SECOND_TRIP_RUNS))
def test_every_tile_takes_a_ragged_second_trip(run):
    w, h, f = cases.SECOND_TRIP_RUNS[run]
    ws, hs = f * w, f * h
    tx, ty = cases.SECOND_TRIP_GRID
    n = geo.clahe_tile_pixels(tx, ty, ws, hs)
    per_tile = geo.clahe_per_tile(tx, ty, ws, hs)
    assert per_tile == 16 and n.min() >= 262 * 251 == 65762 > per_tile * geo.kHistChunk
    assert (n == cnp.tile_luts(np.zeros((hs, ws), np.uint16), cnp.clahe(tx, ty, 0, 8))[1]).all()
    assert (geo.clahe_trips(tx, ty, ws, hs) == 2).all()
    assert ((n - per_tile * geo.kHistChunk) % geo.kHistThreads != 0).all()  # the second trip ends inside a row of lanes
    local = geo.clahe_local_index(tx, ty, ws, hs)
    tiles = cnp.tile_map(ws, hs, tx, ty)
    for t in (0, 9, 63):                                                    # a numbering: 0 .. n - 1 once each inside a tile
        assert (np.sort(local[tiles == t]) == np.arange(n.reshape(-1)[t])).all()
    trip = geo.clahe_trip_map(tx, ty, ws, hs)
    assert set(np.unique(trip)) == {0, 1} and ((trip == 1) == (local >= 65536)).all()


@pytest.mark.parametrize("kernel", ["tone", "clahe"])
@pytest.mark.parametrize("run", list(cases.SECOND_TRIP_RUNS))
def test_late_quarters_sits_where_the_second_trip_reads(run, kernel):
    w, h, f = cases.SECOND_TRIP_RUNS[run]
    ws, hs = f * w, f * h
    px = cases.second_trip_frame(run, kernel)
    assert px.shape == (hs, ws) and not px.flags.writeable
    trip = geo.tone_hist_trip_map(ws, hs) if kernel == "tone" else geo.clahe_trip_map(*cases.SECOND_TRIP_GRID, ws, hs)
    early, late = px[trip == 0], px[trip > 0]
    assert early.max() < 1 << 15 and late.min() >= cases.LATE_FLOOR
    assert {int(v) >> 14 for v in np.unique(early)} == {0, 1} and {int(v) >> 14 for v in np.unique(late)} == {3}
    lo, hi = cases.LATE_RANGE
    assert 0 < (late > hi).sum() < late.size // 10 and 0 < (early < lo).sum() < early.size // 10
    if kernel == "clahe":                                                   # ... in every tile
        tiles = cnp.tile_map(ws, hs, *cases.SECOND_TRIP_GRID)
        bad_late = np.bincount(tiles[(trip > 0) & (px > hi)], minlength=64)
        assert (bad_late > 0).all() and (np.bincount(tiles[trip > 0], minlength=64) > bad_late).all()
    # the range is in the statistics, and at 14 bits the late values all saturate into M
    assert (vnp.histogram(px, 16, cases.LATE_RANGE) != vnp.histogram(px, 16, vnp.OFF)).any()
    assert vnp.histogram(px, 14, cases.LATE_RANGE)[16383] >= (late <= hi).sum() > 0
