"""Python mirror of the launch geometry of the deep intake's kernels (nmi_unpack.hip, nmi_tone.hip, nmi_clahe.hip, plain and
valid-range instantiations alike) -- TEST INFRASTRUCTURE ONLY.

Which lane, block column, chunk and trip of a loop a pixel falls to decides which branch of a kernel a test runs.  The tests of
tests/test_packed_seams.py, tests/test_valid_seams.py and the second-trip cases choose their sizes by these functions, and
tests/test_intake_geometry.py holds the constants against the kernels' sources and proves each size's premise on the CPU.

    unpack       a lane takes a run of 8 container pixels, kUnpackLanes lanes make a block row: 512 pixels per block column
    conversion   a lane makes a quad of 4 output pixels, kBlockRowLanes lanes a block row: 256 output pixels per block column
    tone hist    work item = one run of kHistRun pixels of a row, row-major; a workgroup of kHistThreads lanes takes
                 kHistRunsPerLane runs per lane and trip; at most kHistMaxWorkgroups workgroups
    CLAHE hist   a tile's pixels numbered row-major inside the tile, chunks of kHistThreads * kHistPerLane of them; per_tile
                 workgroups a tile, workgroup c on chunks c, c + per_tile, ...
"""
import numpy as np

kUnpackLanes = 64            # nmi_unpack.hip: lanes (runs) per block row
kUnpackRun = 8               # container pixels per lane
kBlockRowLanes = 64          # nmi_tone.hip / nmi_clahe.hip conversions: lanes (quads) per block row
kQuad = 4                    # output pixels per lane
kHistThreads = 256           # both histogram kernels
kHistRun = 8                 # nmi_tone.hip: pixels of a work item
kHistRunsPerLane = 2         # nmi_tone.hip: work items a lane holds per trip
kHistPerLane = 16            # nmi_clahe.hip: pixels a lane holds per trip
kHistMaxWorkgroups = 1024    # both histogram launchers
kHistChunk = kHistThreads * kHistPerLane   # nmi_clahe.hip: pixels of a chunk


def ceil_div(a, b):
    return -(-a // b)


# --- nmi_unpack.hip -----------------------------------------------------------------------------------------------------------------

def unpack_runs(width):
    return ceil_div(width, kUnpackRun)


def unpack_blocks(width):
    """Block columns of the launch: blockIdx.x runs over 0 .. this - 1."""
    return ceil_div(unpack_runs(width), kUnpackLanes)


def unpack_tail(width):
    """n of the row's last run: 8 for a whole one."""
    return width - kUnpackRun * (unpack_runs(width) - 1)


def unpack_vec(base, width):
    """store_run's path from the container's base address (mod 16 is all that counts) and its width: 2, 1 or 0."""
    if base % 16 == 0 and width % 8 == 0:
        return 2
    if base % 8 == 0 and width % 4 == 0:
        return 1
    return 0


def unpack_tail_bytes(width, group_pixels, group_bytes):
    """Source bytes of the last run of a row (nb of the kernel's byte loop when the run is partial)."""
    n = unpack_tail(width)
    assert n % group_pixels == 0
    return n // group_pixels * group_bytes


# --- the conversions ----------------------------------------------------------------------------------------------------------------

def convert_quads(width):
    return ceil_div(width, kQuad)


def convert_blocks(width):
    return ceil_div(convert_quads(width), kBlockRowLanes)


def convert_tail(width):
    """n of the row's last quad: 4 for a whole one."""
    return width - kQuad * (convert_quads(width) - 1)


def convert_block_of(x):
    """The block column that makes output pixel x."""
    return x // (kQuad * kBlockRowLanes)


# --- nmi_tone.hip's histogram ---------------------------------------------------------------------------------------------------------

def tone_hist(width, height):
    """(items, workgroups, trips) of a width x height source: trips is how often the `first += chunk` loop runs."""
    items = ceil_div(width, kHistRun) * height
    per = kHistThreads * kHistRunsPerLane
    workgroups = min(max(ceil_div(items, per), 1), kHistMaxWorkgroups)
    return items, workgroups, ceil_div(items, workgroups * per)


def tone_hist_trip_map(width, height):
    """[height, width] the trip of the loop on which each pixel is loaded."""
    runs = ceil_div(width, kHistRun)
    _, workgroups, _ = tone_hist(width, height)
    chunk = workgroups * kHistThreads * kHistRunsPerLane
    item = np.arange(height, dtype=np.int64)[:, None] * runs + np.arange(width, dtype=np.int64)[None, :] // kHistRun
    return item // chunk


# --- nmi_clahe.hip's histogram --------------------------------------------------------------------------------------------------------

def clahe_edges(tiles, size):
    """The host's clahe_edges: tile i of an axis holds the coordinates [edge[i], edge[i + 1])."""
    return [0] + [(2 * size * i - tiles + 2 * tiles - 1) // (2 * tiles) for i in range(1, tiles)] + [size]


def clahe_per_tile(tx, ty, width, height):
    """Workgroups per tile (gridDim.x of the launch)."""
    widest, tallest = ceil_div(width, tx) + 1, ceil_div(height, ty) + 1
    chunks = ceil_div(widest * tallest, kHistChunk)
    return min(chunks, kHistMaxWorkgroups // (tx * ty))


def clahe_tile_pixels(tx, ty, width, height):
    """int64 [ty, tx] pixels per tile."""
    ex, ey = np.diff(clahe_edges(tx, width)), np.diff(clahe_edges(ty, height))
    return (ey[:, None] * ex[None, :]).astype(np.int64)


def clahe_trips(tx, ty, width, height):
    """int64 [ty, tx]: the trips workgroup 0 of each tile makes -- the most of any of the tile's workgroups."""
    chunks = -(-clahe_tile_pixels(tx, ty, width, height) // kHistChunk)
    return -(-chunks // clahe_per_tile(tx, ty, width, height))


def clahe_local_index(tx, ty, width, height):
    """[height, width] each pixel's index inside its tile: row of the tile * tile width + column of the tile."""
    ex, ey = np.array(clahe_edges(tx, width)), np.array(clahe_edges(ty, height))
    x, y = np.arange(width, dtype=np.int64), np.arange(height, dtype=np.int64)
    ti, tj = np.searchsorted(ex, x, side="right") - 1, np.searchsorted(ey, y, side="right") - 1
    tw = np.diff(ex)[ti]
    return (y - ey[tj])[:, None] * tw[None, :] + (x - ex[ti])[None, :]


def clahe_trip_map(tx, ty, width, height):
    """[height, width] the trip of its workgroup's loop on which each pixel is loaded."""
    return clahe_local_index(tx, ty, width, height) // kHistChunk // clahe_per_tile(tx, ty, width, height)
