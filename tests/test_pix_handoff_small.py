"""The pixel-range hand-off at its corners (csrc/nmi_pix_device.h: pix_publish / pix_collect, the dealing of pieces): frames of
one to five pieces, so that some or all helpers of a candidate have nothing to publish, row tails of 1 and 9 pixels, a last
piece of 4 chunks, and a single candidate -- on all nine instantiations of nmi_pix_kernel, nmi_masked_pix_kernel and
nmi_covered_pix_kernel.  Rating tables compared with == on the bits against the oracle's rounded mode (plain) and its numpy
restatements (tests/helpers/masked_np.py, covered_np.py), as tests/test_pix_kernel.py and tests/test_covered_pix.py do."""
import numpy as np
import pytest

from helpers import covered_np as cnp
from helpers import masked_np as mnp
from oracle import binding as oc
from orbslam2_nmi_amd import capi
from test_covered_pix import bits, dev

torch = pytest.importorskip("torch")

# (width, height) -> (16-byte chunks, pieces of 64 chunks, pixels of a row's tail, chunks of the last piece); what each is here for
FRAMES = {
    (41, 19): (38, 1, 9, 38),    # every helper is empty; row tails of 9 pixels
    (32, 64): (128, 2, 0, 64),   # aligned rows
    (48, 85): (255, 4, 0, 63),   # fewer pieces than 5 ranges
    (33, 130): (260, 5, 1, 4),   # row tails of 1 pixel; a last piece of 4 chunks
}
GRIDS = [(3, 2), (1, 1)]         # renders x warps; 1 x 1: the kernels' total == 1 branch
RANGES = [2, 3, 4, 5]
SETTINGS = {"256-bg": (256, True), "256-nobg": (256, False), "64-bg": (64, True)}  # bins, background rule: <ZERO0, SHIFTED> = <0,0>, <1,0>, <0,1>
FORMS = ["plain", "masked", "covered"]


def test_frames_are_the_corners_they_are_named_for():
    """The chunk and piece counts of the table above, from the shapes (a piece: 64 chunks of 16 pixels, rows' tails apart)."""
    for (w, h), (chunks, pieces, tail, last) in FRAMES.items():
        assert h * (w // 16) == chunks and -(-chunks // 64) == pieces, (w, h)
        assert w % 16 == tail and chunks - 64 * (pieces - 1) == last, (w, h)
        assert w >= 32 and w * h < 65536  # the kernels' least width; no 16-bit counter can wrap
    assert [FRAMES[k][1] for k in FRAMES] == [1, 2, 4, 5]


@pytest.fixture(scope="module")
def device():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    capi.load_library()  # raises if the HIP library is missing: there is no fallback


def stacks(w, h, S, Wn):
    """Random images with raw zeros in both (the background rule has something to drop) and masks about half set."""
    rng = np.random.default_rng(w * 1000 + h * 10 + S)
    rs = rng.integers(0, 256, (S, h, w), dtype=np.uint8)
    ws = rng.integers(0, 256, (Wn, h, w), dtype=np.uint8)
    rs[:, : h // 4, : w // 3] = 0
    ws[:, h // 6: h // 2, w // 5: w // 2] = 0
    wm = (rng.random((Wn, h, w)) < 0.5).astype(np.uint8) * rng.integers(1, 4, (Wn, h, w)).astype(np.uint8)  # any nonzero byte means "set"
    rm = (rng.random((S, h, w)) < 0.5).astype(np.uint8)
    return rs, ws, wm, rm


def model(form, rs, ws, wm, rm, shift, use_bg, bottom_up):
    """-> (ratings, index, score, counts or None)"""
    if form == "plain":
        with oc.rounded():
            return (*oc.search_grid(rs, ws, render_bottom_up=bottom_up, threads=4, use_bg=use_bg, shift=shift), None)
    if form == "masked":
        return (*mnp.masked_search(rs, ws, wm, shift, use_bg, bottom_up), np.count_nonzero(wm.reshape(len(wm), -1), axis=1))
    return cnp.covered_search(rs, ws, wm, rm, shift, use_bg, bottom_up)


def search(ctx, form, d, S, Wn):
    """One search of `form` on the device stacks d -> (ratings, index, score, counts or None)."""
    t = torch.full((Wn, S), -3.0, device="cuda")
    if form == "plain":
        idx, best = ctx.search_grid(d["rs"], d["ws"], t)
        counts = None
    elif form == "masked":
        idx, best = ctx.search_grid_masked(d["rs"], d["ws"], d["wm"], t)
        counts = ctx.mask_counts(Wn)
    else:
        idx, best = ctx.search_grid_covered(d["rs"], d["rm"], d["ws"], d["wm"], t)
        counts = ctx.cover_counts(S * Wn).reshape(Wn, S)
    return t.cpu().numpy(), idx, best, counts


def check(got, want, what):
    assert (bits(got[0]) == bits(want[0])).all(), what
    assert (got[1], bits(got[2])) == (want[1], bits(want[2])), what
    if want[3] is not None:
        assert np.array_equal(got[3], want[3]), what


@pytest.mark.gpu
@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: f"{g[0]}x{g[1]}")
@pytest.mark.parametrize("frame", list(FRAMES), ids=lambda f: f"{f[0]}x{f[1]}")
def test_small_frames_on_forced_ranges(device, frame, grid, setting):
    """Every form on P = 2 .. 5 forced ranges: the model's bits, winner and counts, P ranges launched, nothing healed."""
    (w, h), (S, Wn), (bins, use_bg) = frame, grid, SETTINGS[setting]
    bottom_up = w % 16 != 0  # the frames with row tails against bottom-up renders, the aligned ones against top-down ones
    rs, ws, wm, rm = stacks(w, h, S, Wn)
    want = {form: model(form, rs, ws, wm, rm, {256: 0, 64: 2}[bins], use_bg, bottom_up) for form in FORMS}
    d = {"rs": dev(rs), "ws": dev(ws), "wm": dev(wm), "rm": dev(rm)}
    with capi.NmiContext(w, h, bins=bins, use_bg=use_bg, render_bottom_up=bottom_up) as ctx:
        ctx.set_option(ctx.OPT_SPLIT, 1)
        for P in RANGES:
            ctx.set_option(ctx.OPT_SPLIT_PIXELS, P)
            for form in FORMS:
                got = search(ctx, form, d, S, Wn)
                assert ctx.pix_status() == {"last_launch_ranges": P, "healed": 0}, (form, P)
                assert ctx.pix_heal_counts() == {"timeouts": 0, "count_test": 0}, (form, P)  # (no field can wrap: a redo would be a stale hand-off)
                check(got, want[form], (form, P))


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_a_withheld_hand_off_heals_on_a_frame_of_one_piece(device, form):
    """41x19, 3 ranges, phase-mask bit 9: helper 1 of every candidate (which has no pixels, like helper 2) keeps its tags to
    itself, every owner gives up after its bounded wait and scores its candidate alone on the exact path: the same bits."""
    w, h, S, Wn = 41, 19, 3, 2
    rs, ws, wm, rm = stacks(w, h, S, Wn)
    want = model(form, rs, ws, wm, rm, 0, True, True)
    d = {"rs": dev(rs), "ws": dev(ws), "wm": dev(wm), "rm": dev(rm)}
    with capi.NmiContext(w, h) as ctx:
        ctx.set_option(ctx.OPT_SPLIT, 1)
        ctx.set_option(ctx.OPT_SPLIT_PIXELS, 3)
        ctx.set_option(ctx.OPT_PHASE_MASK, 3 | 512)
        got = search(ctx, form, d, S, Wn)
        assert ctx.pix_status() == {"last_launch_ranges": 3, "healed": S * Wn}
        assert ctx.pix_heal_counts() == {"timeouts": S * Wn, "count_test": 0}
        check(got, want, form)
