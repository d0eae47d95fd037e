"""The hand-offs between workgroups of one launch -- nmi_split_kernel's, and pix_publish / pix_collect of the three pixel-range
kernels (csrc/nmi_pix_device.h) -- where a stale read would otherwise stay unseen: on blocks that the previous launch left holding
OTHER content, and on a chip that another context keeps unevenly busy.

Scoring frames are 128 x 96: 768 chunks = 12 pieces, so that on up to 5 ranges every helper has pixels to publish, and 12,288
pixels, so that no 16-bit field can wrap: a count-test redo (nmi_pix_heal_counts) on these frames can only be a hand-off that
was read stale -- a unit, a side counter or a header word short -- which the owner would otherwise heal without a trace.  The
split kernel has 32-bit counters and no count test: there stale data shows in the bits.  Every launch is compared with its model
(the oracle's rounded mode, tests/helpers/masked_np.py, covered_np.py) with == on the bits, plus winner and counts.

A timeout (an owner that gave up a 2 ms wait because its helper found no compute unit) is legitimate under load and never fails a
test; the tests under load only insist that most launches did go through a hand-off, or they say that nothing was exercised."""
import functools
import threading
import time

import numpy as np
import pytest

from helpers import pix_ranges_np as prn
from oracle import binding as oc
from orbslam2_nmi_amd import capi
from test_covered_pix import bits, dev
from test_pix_handoff_small import check, model, search, stacks

torch = pytest.importorskip("torch")

W, H = 128, 96
S_MAX, WN_MAX = 8, 5
FORMS = ["plain", "masked", "covered"]
SETS = {"plain": "ABC", "masked": "AB", "covered": "AB"}  # C folds flat chunks into side counters: the plain kernel only
C1_GRIDS = [(3, 2), (2, 3), (6, 1)]  # renders x warps: 6 candidates each, so every launch reuses the same 6 x (P - 1) blocks


def test_scoring_frames_make_every_helper_publish_and_no_field_wrap():
    chunks = H * (W // 16)
    assert W % 16 == 0 and chunks == 768 and -(-chunks // 64) == 12
    assert W * H == 12288 < 65536  # no 16-bit field can wrap: a count-test redo is a stale hand-off
    for P in (2, 3, 4, 5):
        ranges = prn.range_of_pixels(W, H, P)
        assert sorted(np.unique(ranges)) == list(range(P)), P  # every helper has pixels of its own


@functools.lru_cache(maxsize=None)
def content(name):
    """-> (renders [8], warps [5], warp masks, render masks) of a content set, on the host."""
    if name == "B":  # zeros blocked in: the background rule has something to drop; masks about half set
        return stacks(W, H, S_MAX, WN_MAX)
    rng = np.random.default_rng({"A": 101, "C": 303}[name])
    rs = rng.integers(1, 256, (S_MAX, H, W), dtype=np.uint8)
    ws = rng.integers(1, 256, (WN_MAX, H, W), dtype=np.uint8)
    if name == "C":  # bands of distinct flat pairs down the image: every range meets several, more than an owner's eight side counters
        for s in range(S_MAX):
            for band in range(12):
                rs[s, band * 8:band * 8 + 5, :] = 255 - (band % 11) * (s % 3 + 1)
        for v in range(WN_MAX):
            for band in range(12):
                ws[v, band * 8:band * 8 + 5, :] = (band * 17 + v) % 256
    wm = (rng.random((WN_MAX, H, W)) < 0.5).astype(np.uint8) * rng.integers(1, 4, (WN_MAX, H, W)).astype(np.uint8)
    rm = (rng.random((S_MAX, H, W)) < 0.5).astype(np.uint8)
    return rs, ws, wm, rm


@functools.lru_cache(maxsize=None)
def expected(form, name, S, Wn):
    """The model of a search of `form` over the first S renders and Wn warps of a set (computed once, never changed)."""
    rs, ws, wm, rm = content(name)
    return model(form, rs[:S], ws[:Wn], wm[:Wn], rm[:S], 0, True, True)


@functools.lru_cache(maxsize=None)
def expected_pair(name, s, v):
    rs, ws, _, _ = content(name)
    with oc.rounded():
        return oc.eval_pair(rs[s], ws[v])


@pytest.fixture(scope="module")
def device():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    capi.load_library()  # raises if the HIP library is missing: there is no fallback
    return {name: dict(zip(("rs", "ws", "wm", "rm"), (dev(a) for a in content(name)))) for name in "ABC"}


def sub(d, S, Wn):
    return {"rs": d["rs"][:S], "ws": d["ws"][:Wn], "wm": d["wm"][:Wn], "rm": d["rm"][:S]}


def split_launch(ctx, device, i, grid):
    """Launch i of a split-kernel sequence, sets A and B in turn: a 3 x 3 grid, or a single pair that moves through the set."""
    name = "AB"[i % 2]
    d = device[name]
    if grid:
        got = search(ctx, "plain", sub(d, 3, 3), 3, 3)
        check(got, expected("plain", name, 3, 3), ("split 3x3", name, i))
    else:
        s, v = i % S_MAX, (i // 2) % WN_MAX
        assert bits(ctx.eval_pair(d["rs"][s], d["ws"][v])) == bits(expected_pair(name, s, v)), ("split pair", name, s, v, i)
    return ctx.split_status()["last_launch_parts"]


@pytest.mark.gpu
@pytest.mark.parametrize("P", [2, 5])
@pytest.mark.parametrize("form", FORMS)
def test_reused_blocks_with_changing_content(device, form, P):
    """60 launches on one context, forced to P ranges, cycling through the content sets and through three shapes of a
    6-candidate grid: the block that served candidate i of one set serves another candidate of another set in the next launch,
    so a line or a block that survived from the launch before holds a wrong value, not a matching one."""
    with capi.NmiContext(W, H) as ctx:
        ctx.set_option(ctx.OPT_SPLIT, 1)
        ctx.set_option(ctx.OPT_SPLIT_PIXELS, P)
        for i in range(60):
            name, (S, Wn) = SETS[form][i % len(SETS[form])], C1_GRIDS[(i // len(SETS[form])) % 3]
            got = search(ctx, form, sub(device[name], S, Wn), S, Wn)
            assert ctx.pix_status()["last_launch_ranges"] == P, i
            check(got, expected(form, name, S, Wn), (form, P, name, S, Wn, i))
        assert ctx.pix_heal_counts() == {"timeouts": 0, "count_test": 0}


@pytest.mark.gpu
def test_split_kernel_reuses_blocks_with_changing_content(device):
    """The row-split kernel in automatic mode: single pairs that move through the sets, and 3 x 3 grids, sets A and B in turn."""
    with capi.NmiContext(W, H) as ctx:
        for i in range(60):
            assert split_launch(ctx, device, i, grid=i % 4 >= 2) > 0, i
        assert ctx.split_status()["timeouts"] == 0


# ---- under load ---------------------------------------------------------------------------------------------------------------

LOADS = {"steady": (30, 20), "pulsed": (10, 10)}  # renders x warps of the loader's searches: 600 / 100 candidates at 640 x 480


@functools.lru_cache(maxsize=None)
def loader_content(kind):
    S, Wn = LOADS[kind]
    rng = np.random.default_rng(S)
    rs = rng.integers(0, 256, (S, 480, 640), dtype=np.uint8)
    ws = rng.integers(0, 256, (Wn, 480, 640), dtype=np.uint8)
    with oc.rounded():
        _, io, bo = oc.search_grid(rs, ws, threads=16)
    return rs, ws, (io, bo)


class Loader(threading.Thread):
    """A second context at 640 x 480 that keeps part of the chip busy with blocking searches until told to stop, and checks its
    own winner every time.  steady: 600 candidates on 3/8 of the compute units, back to back.  pulsed: 100 candidates on 61
    workgroups (no multiple of the 8 XCDs) with a short random pause in between, so that compute units free up and fill again
    in the middle of the scorer's launches."""

    def __init__(self, kind):
        super().__init__(daemon=True)
        self.kind, self.done, self.errors = kind, 0, []
        self.started, self.stop = threading.Event(), threading.Event()
        rs, ws, self.expect = loader_content(kind)
        self.rs, self.ws = dev(rs), dev(ws)

    def run(self):
        rng = np.random.default_rng(7)
        try:
            with capi.NmiContext(640, 480) as ctx:
                ctx.set_option(ctx.OPT_WORKGROUPS, 61 if self.kind == "pulsed" else ctx.info()["compute_units"] * 3 // 8)
                while not self.stop.is_set():
                    got = ctx.search_grid(self.rs, self.ws)
                    if got != self.expect:
                        self.errors.append(("loader winner", self.done, got, self.expect))
                        break
                    self.done += 1
                    self.started.set()
                    if self.kind == "pulsed":
                        time.sleep(rng.uniform(0.0, 2e-4))
        except Exception as e:  # noqa: BLE001
            self.errors.append(repr(e))
        finally:
            self.started.set()

    def __enter__(self):
        self.start()
        self.started.wait()  # the scorer starts only after the loader's first search
        return self

    def __exit__(self, *exc):
        self.stop.set()
        self.join()


def split_steps(ctx, device, cap, tally):
    for grid in (False, True):
        for i in range(120):
            before = ctx.split_status()["timeouts"]
            parts = split_launch(ctx, device, i, grid)
            timed_out = ctx.split_status()["timeouts"] - before
            tally["launches"] += 1
            tally["split_launches"] += 1
            tally["split_timeouts"] += timed_out
            tally["handed_off"] += int(parts > 0 and not timed_out)


def pix_steps(form):
    def steps(ctx, device, cap, tally):
        # automatic mode: 8 x 5 = 40 candidates (3 ranges on half of 256 compute units); then forced to 5 ranges, on the
        # largest S x 5 grid whose S * 5 * 5 workgroups fit the scorer's cap (5 x 5 on half of 256 compute units)
        forced_S = max(1, min(S_MAX, cap // 25))
        for forced, (S, Wn) in ((False, (S_MAX, WN_MAX)), (True, (forced_S, WN_MAX))):
            ctx.set_option(ctx.OPT_SPLIT, 1 if forced else -1)
            ctx.set_option(ctx.OPT_SPLIT_PIXELS, 5 if forced else -1)
            for i in range(120):
                name = SETS[form][i % len(SETS[form])]
                before = ctx.pix_heal_counts()["timeouts"]
                got = search(ctx, form, sub(device[name], S, Wn), S, Wn)
                ranges, timed_out = ctx.pix_status()["last_launch_ranges"], ctx.pix_heal_counts()["timeouts"] - before
                check(got, expected(form, name, S, Wn), (form, "forced" if forced else "auto", name, i))
                assert ranges == 5 or not forced, (form, i, ranges)
                tally["launches"] += 1
                tally["pix_candidates"] += S * Wn
                tally["pix_timeouts"] += timed_out
                tally["handed_off"] += int(ranges > 0 and not timed_out)
    return steps


STEPS = {"split": split_steps, "plain": pix_steps("plain"), "masked": pix_steps("masked"), "covered": pix_steps("covered")}


@pytest.mark.gpu
@pytest.mark.parametrize("step", list(STEPS))
@pytest.mark.parametrize("load", list(LOADS))
def test_hand_offs_under_uneven_load(device, load, step):
    """240 scoring launches (120 pairs + 120 3 x 3 grids of the split kernel, or 120 automatic + 120 forced-to-5-ranges searches of
    a pixel-range form) on a context capped at half the compute units, while the loader runs beside it.  Every bit, winner and
    count equals the model and no merged decode failed the count test.  Timeouts are allowed, but the test says so when the
    hand-off was not exercised: the loader must complete 20 searches between the scorer's first and last launch, and 90 % of the
    scoring launches must go through a hand-off form without a timeout, with timeouts at no more than 10 % of the pixel-range
    candidates / of the split launches."""
    tally = dict.fromkeys(("launches", "handed_off", "pix_candidates", "pix_timeouts", "split_launches", "split_timeouts"), 0)
    with Loader(load) as loader:
        with capi.NmiContext(W, H) as ctx:
            cap = ctx.info()["compute_units"] // 2
            ctx.set_option(ctx.OPT_WORKGROUPS, cap)
            first = loader.done
            STEPS[step](ctx, device, cap, tally)
            beside = loader.done - first
            counts = ctx.pix_heal_counts()
    print(f"{load}/{step}: {tally}, heal counts {counts}, loader searches beside the scorer {beside}")
    assert not loader.errors, loader.errors
    assert counts["count_test"] == 0, counts
    not_exercised = f"the hand-off was not exercised under load: {tally}, loader searches beside the scorer: {beside}"
    assert beside >= 20, not_exercised
    assert tally["handed_off"] >= 0.9 * tally["launches"], not_exercised
    assert tally["pix_timeouts"] <= 0.1 * tally["pix_candidates"] and tally["split_timeouts"] <= 0.1 * tally["split_launches"], not_exercised


@pytest.mark.gpu
def test_captured_level_under_steady_load(device):
    """The 9 x 9 captured level of tests/test_pix_kernel.py, replayed 24 times with views, warps and camera frame alternating
    between two settings while the steady loader runs: every replay's table is the oracle's on the stacks that replay produced,
    and no merged decode failed the count test -- which no wrap can explain: a joint bin holds at most what the fuller of its
    two intensities holds in either image, and that stays below 65,536 in every replay's stacks."""
    import orbslam2_nmi_amd as nmi
    from test_pix_kernel import replay_captured_mid_size_level
    with Loader("steady") as loader:
        first = loader.done
        st = replay_captured_mid_size_level(nmi, 24, lambda rep: (1.0, 1.6)[rep % 2], frame_shifts=((0.05, 0, 0), (-0.04, 0.03, 0)))
        beside = loader.done - first
    print(f"captured level under steady load: {st}, loader searches beside the replays {beside}")
    assert not loader.errors, loader.errors
    assert st["largest_bin_bound"] < 65536  # (the premise)
    assert st["count_test"] == 0, st
    assert beside >= 20, f"the level was not replayed under load: loader searches beside the replays: {beside}"
