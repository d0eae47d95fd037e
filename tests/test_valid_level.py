"""GPU tests (-m gpu) of the valid range of captured levels (nmi_level_set_valid_range, include/nmi_hip.h), on a small point cloud
with S = 3, Wn = 3 at 64x48, 52x38 (frame rows not 16-byte aligned: the warp kernel on the forked branch) and 54x38 (W % 4 != 0:
the conversion's scalar output path).

The baseline is always a second level fed the numpy twin's 8-bit frame as plain grey (tests/helpers/valid_np.py: deep_frame) and,
masked or covered, the twin's validity mask as its d_frame_mask -- with a lens, both as raw.  Winner, score bits and the rating
table are ==, warps byte-equal, warp masks and counts byte-equal through nmi_level_copy_masks / _copy_coverage.  Each case also
asserts that the rating table under the range differs from the same level's without it (where the header's rule lets it: a plain
level under SHIFT takes the statistics only and SHIFT has none, so there the two are asserted equal)."""
import numpy as np
import pytest

from helpers import fisheye_np as fnp
from helpers import packed_np as pnp
from helpers import tone_np as tnp
from helpers import undistort_np as unp
from helpers import valid_np as vnp
from helpers import valid_pipeline_cases as cases
from orbslam2_nmi_amd import capi, sharding
from test_color_level import bits, enable, lens_K, scene
from test_fisheye_level import raw_K
from test_masked_level import compose, dev, views, warps
from test_packed_frame import dev16, dev_at
from test_packed_level import deep as deep_fmt

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

S, WN = 3, 3
RADTAN = unp.FAMILIES["barrel"]
FISHEYE = fnp.FAMILIES["euroc_eq"]
RANGE = cases.RANGE
E = capi.ERR_INVALID_ARGUMENT


@pytest.fixture(scope="module")
def nmi():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    import orbslam2_nmi_amd as m
    m.load_library()
    return m


def replay(lv, kind, mvps, Ms):
    """-> (winner, [ratings, warps, then the masked / covered level's warp masks and counts])"""
    win = lv.run(mvps, Ms)
    _, ws, t = lv.outputs()
    out = [t.copy(), ws.copy()]
    if kind == "masked":
        out += [a.copy() for a in lv.masks()]
    elif kind == "covered":
        out += [a.copy() for a in lv.coverage()]
    return win, out


def same_replay(a, b):
    assert a[0][0] == b[0][0], (a[0], b[0])
    assert bits(np.float32(a[0][1])) == bits(np.float32(b[0][1])), (a[0], b[0])
    assert len(a[1]) == len(b[1])
    for x, y in zip(a[1], b[1]):
        assert x.shape == y.shape and x.dtype == y.dtype
        assert (np.ascontiguousarray(x).view(np.uint8) == np.ascontiguousarray(y).view(np.uint8)).all()


def off_one(mask):
    """The mask on the device at an address 1 byte off 4-byte alignment."""
    h, w = mask.shape
    t = torch.zeros(h * w + 8, dtype=torch.uint8, device="cuda")
    start = (-t.data_ptr()) % 4 + 1
    v = t[start:start + h * w].view(h, w)
    v.copy_(dev(mask))
    assert v.data_ptr() % 4 == 1
    return v


def set_lens(lv, lens, K, w):
    if lens == "radtan":
        lv.set_distortion(K, RADTAN)
    elif lens == "fisheye":
        lv.set_distortion_fisheye(K, raw_K(K, w), FISHEYE)


class Pair:
    """A GRAY16 level under test on the planted pipeline frame, and the baseline level on the twin's grey frame and mask."""

    def __init__(self, nmi, ctx, sc, w, h, kind, f, lens, hood, seed=0):
        self.w, self.h, self.kind, self.f = w, h, kind, f
        self.gray0 = sc.frame.cpu().numpy()
        self.pitch, self.off = 2 * f * w + 10, 2
        self.px = cases.frame(self.gray0, f, seed)
        cases.premises(self.px, f)
        self.d = dev(tnp.pack16(self.px, self.pitch, self.off, seed=2))
        self.fm = cases.hood(w, h) if hood else None
        self.d_fm = off_one(self.fm) if hood else None
        self.fm_was = None if self.d_fm is None else self.d_fm.cpu().numpy().copy()
        self.twin_frame, self.twin_mask = dev(np.zeros((h, w), np.uint8)), dev(np.zeros((h, w), np.uint8))
        self.lv = nmi.NmiLevel(ctx, sc.dx, sc.da, self.d[self.off:], S, WN, 3.0)
        self.base = nmi.NmiLevel(ctx, sc.dx, sc.da, self.twin_frame, S, WN, 3.0)
        K = lens_K(sc.rp)
        self.lv.set_frame_reduction(f, capi.FRAME_GRAY16, self.pitch)
        enable(self.lv, kind, self.d_fm)
        enable(self.base, kind, self.twin_mask)
        for target in (self.lv, self.base):
            set_lens(target, lens, K, w)

    def refill(self, px):
        self.px = px
        self.d.copy_(dev(tnp.pack16(px, self.pitch, self.off, seed=2)))
        torch.cuda.synchronize()

    def twin(self, tm, rng):
        gray, mask = vnp.deep_frame(self.px, self.f, tm, rng, self.fm)
        self.twin_frame.copy_(dev(gray))
        self.twin_mask.copy_(dev(mask))
        torch.cuda.synchronize()

    def close(self):
        if self.d_fm is not None:                                     # the caller's frame mask is only ever read
            assert (self.d_fm.cpu().numpy() == self.fm_was).all()
        self.lv.close()
        self.base.close()


def differs(kind, label, on, off):
    """The range must have changed the replay -- except where the header says it cannot: a plain level takes the statistics only,
    and SHIFT has none."""
    if kind == "plain" and label == "shift":
        assert (bits(on[1][0]) == bits(off[1][0])).all()
    else:
        assert (bits(on[1][0]) != bits(off[1][0])).any(), (kind, label)


# kind, factor, lens, hood mask
VARIANTS = {"plain": ("plain", 1, None, False), "masked-null": ("masked", 1, None, False), "masked-hood": ("masked", 1, None, True),
            "covered": ("covered", 1, None, True), "masked-f2": ("masked", 2, None, False), "plain-f2": ("plain", 2, None, False),
            "masked-radtan": ("masked", 1, "radtan", True), "masked-f2-fisheye": ("masked", 2, "fisheye", True),
            "covered-radtan": ("covered", 1, "radtan", False), "covered-f2-fisheye": ("covered", 2, "fisheye", True)}


@pytest.mark.parametrize("size", cases.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_a_ranged_level_equals_the_level_on_the_twins_frame_and_mask(nmi, variant, size):
    w, h = size
    kind, f, lens, hood = VARIANTS[variant]
    with nmi.NmiContext(w, h) as ctx:
        sc = scene(nmi, ctx, w, h, False, kind)
        mvps, Ms = views(sc.rp, S), warps(w, h, WN)
        p = Pair(nmi, ctx, sc, w, h, kind, f, lens, hood)
        try:
            for label, tm in cases.tone_maps().items():
                p.lv.set_tone_map(cases.capi_tone(capi, tm))
                p.lv.set_valid_range(*RANGE)
                p.twin(tm, RANGE)
                got = replay(p.lv, kind, mvps, Ms)
                same_replay(got, replay(p.base, kind, mvps, Ms))
                same_replay(got, replay(p.lv, kind, mvps, Ms))        # a second replay: histograms and the validity buffer start clean
                p.lv.set_valid_range()                                # off: the parent's level, on the unranged twin
                p.twin(tm, vnp.OFF)
                if kind != "plain":                                   # (range off: the level's frame mask is the caller's again)
                    p.twin_mask.copy_(dev(np.ones((h, w), np.uint8) if p.fm is None else p.fm))
                    torch.cuda.synchronize()
                plain = replay(p.lv, kind, mvps, Ms)
                same_replay(plain, replay(p.base, kind, mvps, Ms))
                differs(kind, label, got, plain)
        finally:
            p.close()


@pytest.mark.parametrize("name", ["mono12p", "bayer16-grbg"])
def test_a_ranged_packed_level_equals_the_gray16_level_on_the_container(nmi, name):
    w, h = 52, 38
    fmt = {"mono12p": pnp.MONO12P, "bayer16-grbg": pnp.BAYER16["grbg"]}[name]
    top = (1 << pnp.BITS[fmt]) - 1
    rng = (1, top - 1)
    words = pnp.GROUP[fmt][1] == 2
    with nmi.NmiContext(w, h) as ctx:
        sc = scene(nmi, ctx, w, h, False, "masked")
        gray0 = sc.frame.cpu().numpy()
        mvps, Ms = views(sc.rp, S), warps(w, h, WN)
        for f in (1, 2):
            px = cases.plant(deep_fmt(cases.spread(gray0, f, f), fmt, f), f, f, sentinel=top)
            pitch, off = pnp.row_bytes(fmt, f * w) + (2 if words else 3), 2 if words else 1
            buf = pnp.frame(px, fmt, pitch, 0, f)
            cont = pnp.container(buf, fmt, f * w, f * h, pitch)
            m = vnp.mask(cont, f, rng)
            assert 0.05 <= 1.0 - float(m.mean()) <= 0.6               # validity is taken on the container
            d, d_cont = dev_at(buf, off), dev16(cont)
            with nmi.NmiLevel(ctx, sc.dx, sc.da, d, S, WN, 3.0) as lv, nmi.NmiLevel(ctx, sc.dx, sc.da, d_cont, S, WN, 3.0) as base:
                lv.set_valid_range(*rng)                              # before the format: kept
                lv.set_frame_reduction(f, fmt, pitch)
                base.set_frame_reduction(f, capi.FRAME_GRAY16, 0)
                base.set_valid_range(*rng)
                for target in (lv, base):
                    target.set_masks(True, None)
                for tm in (capi.ToneMap.shift(pnp.BITS[fmt]), capi.ToneMap.equalize(0, pnp.BITS[fmt])):
                    lv.set_tone_map(tm)
                    base.set_tone_map(tm)
                    got = replay(lv, "masked", mvps, Ms)
                    same_replay(got, replay(base, "masked", mvps, Ms))
                    lv.set_valid_range()
                    plain = replay(lv, "masked", mvps, Ms)
                    lv.set_valid_range(*rng)
                    assert (bits(got[1][0]) != bits(plain[1][0])).any()


def test_the_frame_changes_in_place_down_to_no_valid_pixel(nmi):
    """Holes, then no valid pixel at all (N == 0: the table all 0, the mask all 0), then holes again, in place in the level's
    frame.  What a masked search returns on all-zero warp masks is asked of the standalone search, not stated here."""
    w, h = 64, 48
    tm = cases.tone_maps()["equalize"]
    with nmi.NmiContext(w, h) as ctx:
        sc = scene(nmi, ctx, w, h, False, "masked")
        mvps, Ms = views(sc.rp, S), warps(w, h, WN)
        p = Pair(nmi, ctx, sc, w, h, "masked", 1, None, False)
        try:
            p.lv.set_tone_map(cases.capi_tone(capi, tm))
            p.lv.set_valid_range(*RANGE)
            holes = p.px
            nothing = np.zeros_like(holes)
            nothing[::5, ::7] = 65535
            seen = []
            for px in (holes, nothing, np.roll(holes, 7, axis=1)):
                p.refill(px)
                p.twin(tm, RANGE)
                got = replay(p.lv, "masked", mvps, Ms)
                same_replay(got, replay(p.base, "masked", mvps, Ms))
                seen.append(got)
                if px is nothing:
                    (win, (t, ws, wm, cnt)) = got
                    assert (wm == 0).all() and (cnt == 0).all() and (ws == 0).all()     # table all 0, mask all 0
                    rs = p.lv.outputs()[0]
                    t2 = torch.full(t.shape, -3.0, device="cuda")
                    assert ctx.search_grid_masked(dev(rs), dev(ws), dev(wm), t2) == win
                    assert (bits(t2.cpu().numpy()) == bits(t)).all()
            assert (bits(seen[0][1][0]) != bits(seen[2][1][0])).any()
        finally:
            p.close()


def fresh_replay(nmi, ctx, sc, content, state, K, w, mvps, Ms):
    """A level built directly in `state` on a buffer of its own holding `content`."""
    rng, masked, lens, (f, fmt, pitch), tm = state
    with nmi.NmiLevel(ctx, sc.dx, sc.da, dev(content), S, WN, 3.0) as lv:
        lv.set_tone_map(tm)
        lv.set_frame_reduction(f, fmt, pitch)
        set_lens(lv, lens, K, w)
        if masked:
            lv.set_masks(True, None)
        lv.set_valid_range(*rng)
        return replay(lv, "masked" if masked else "plain", mvps, Ms)


def test_a_level_walks_through_its_settings(nmi):
    """range on -> masks on -> lens on -> range off -> another range -> plain GRAY (the range ignored) -> back: each state replays as
    a fresh level built directly in that state.  Refused arguments and a NULL level in between leave it replaying as before."""
    w, h = 64, 48
    with nmi.NmiContext(w, h) as ctx:
        lib = ctx._lib
        sc = scene(nmi, ctx, w, h, False, "masked")
        K = lens_K(sc.rp)
        gray0 = sc.frame.cpu().numpy()
        mvps, Ms = views(sc.rp, S), warps(w, h, WN)
        tm = cases.capi_tone(capi, cases.tone_maps()["equalize"])
        deep16 = np.ascontiguousarray(cases.frame(gray0, 1, 3), "<u2").view(np.uint8).reshape(-1)
        g16, gray = (1, capi.FRAME_GRAY16, 0), (1, capi.FRAME_GRAY, 0)
        other = (9500, 16383)                                          # the darker third of the band is invalid too
        # (range, masked, lens, frame setting, tone map), what the frame buffer holds then, the one setter that leads there
        walk = [((RANGE, False, None, g16, tm), deep16, lambda lv: lv.set_valid_range(*RANGE)),
                ((RANGE, True, None, g16, tm), deep16, lambda lv: lv.set_masks(True, None)),
                ((RANGE, True, "radtan", g16, tm), deep16, lambda lv: lv.set_distortion(K, RADTAN)),
                ((vnp.OFF, True, "radtan", g16, tm), deep16, lambda lv: lv.set_valid_range()),
                ((other, True, "radtan", g16, tm), deep16, lambda lv: lv.set_valid_range(*other)),
                ((other, True, "radtan", gray, tm), gray0.reshape(-1), lambda lv: lv.set_frame_format(capi.FRAME_GRAY, 0)),
                ((other, True, "radtan", g16, tm), deep16, lambda lv: lv.set_frame_format(capi.FRAME_GRAY16, 0))]
        frame = torch.zeros(deep16.size, dtype=torch.uint8, device="cuda")
        tables = []
        with nmi.NmiLevel(ctx, sc.dx, sc.da, frame, S, WN, 3.0) as lv:
            lv.set_tone_map(tm)
            lv.set_frame_format(capi.FRAME_GRAY16, 0)
            for state, content, step in walk:
                frame[:content.size].copy_(dev(content))
                torch.cuda.synchronize()
                step(lv)
                kind = "masked" if state[1] else "plain"
                got = replay(lv, kind, mvps, Ms)
                same_replay(got, fresh_replay(nmi, ctx, sc, content, state, K, w, mvps, Ms))
                for lo, hi in ((-1, 5), (7, 3), (0, 65536)):
                    assert lib.nmi_level_set_valid_range(lv._h, lo, hi) == E, (lo, hi)
                    with pytest.raises(capi.NmiError):
                        lv.set_valid_range(lo, hi)
                assert lib.nmi_level_set_valid_range(None, *RANGE) == E
                same_replay(got, replay(lv, kind, mvps, Ms))          # as it was
                tables.append(bits(got[1][0]).copy())
        assert (tables[2] != tables[3]).any() and (tables[3] != tables[4]).any() and (tables[4] == tables[6]).all()
        # the range is ignored under plain GRAY: the state equals the same one with the range off
        ignored = fresh_replay(nmi, ctx, sc, gray0.reshape(-1), (vnp.OFF, True, "radtan", gray, tm), K, w, mvps, Ms)
        assert (bits(ignored[1][0]) == tables[5]).all()


def test_the_contexts_range_does_not_reach_a_level(nmi):
    w, h = 52, 38
    tm = cases.tone_maps()["equalize"]
    with nmi.NmiContext(w, h) as ctx:
        sc = scene(nmi, ctx, w, h, False, "masked")
        mvps, Ms = views(sc.rp, S), warps(w, h, WN)
        p = Pair(nmi, ctx, sc, w, h, "masked", 1, None, True)
        try:
            p.lv.set_tone_map(cases.capi_tone(capi, tm))
            before = replay(p.lv, "masked", mvps, Ms)
            ctx.set_tone_map(cases.capi_tone(capi, tm))
            ctx.set_valid_range(*RANGE)
            d_mask = ctx.deep_frame(p.d[p.off:], 1, p.pitch)[1]
            same_replay(before, replay(p.lv, "masked", mvps, Ms))     # the level has no range: as before
            p.lv.set_tone_map(cases.capi_tone(capi, tm))              # ... and a recapture under the context's range changes nothing
            same_replay(before, replay(p.lv, "masked", mvps, Ms))
            p.twin(tm, vnp.OFF)
            p.twin_mask.copy_(dev(p.fm))
            torch.cuda.synchronize()
            same_replay(before, replay(p.base, "masked", mvps, Ms))
            assert (d_mask.cpu().numpy() == vnp.mask(p.px, 1, RANGE)).all()   # the context's own entries do follow it
            ctx.set_valid_range()
            p.lv.set_valid_range(*RANGE)                              # and the level's range does not need the context's
            p.twin(tm, RANGE)
            got = replay(p.lv, "masked", mvps, Ms)
            same_replay(got, replay(p.base, "masked", mvps, Ms))
            assert (bits(got[1][0]) != bits(before[1][0])).any()
        finally:
            p.close()


def test_ranged_blocks_compose_to_the_ranged_level(nmi):
    """Two nmi_level_create_block halves of the grid, masked with the range on: their cells are the whole level's, the MAX of their
    keys its winner; an empty block takes the setting; nmi_level_run_rccl at world size 1 gives the level's winner."""
    w, h, S4 = 64, 48, 4
    tm = cases.capi_tone(capi, cases.tone_maps()["pct"])
    with nmi.NmiContext(w, h) as ctx:
        sc = scene(nmi, ctx, w, h, False, "masked")
        mvps, Ms = views(sc.rp, S4), warps(w, h, WN)
        px = cases.frame(sc.frame.cpu().numpy(), 2, 4)
        d = dev(tnp.pack16(px))
        fm = dev(cases.hood(w, h))

        def level(s, wn, block=None):
            lv = nmi.NmiLevel(ctx, sc.dx, sc.da, d, s, wn, 3.0, block=block)
            lv.set_valid_range(*RANGE)
            lv.set_frame_reduction(2, capi.FRAME_GRAY16, 0)
            lv.set_tone_map(tm)
            lv.set_masks(True, fm)
            return lv

        with level(S4, WN) as full:
            ref = full.run(mvps, Ms)
            t_ref, wm_ref = full.outputs()[2].copy(), full.masks()[0].copy()
            twin_mask = vnp.mask(px, 2, RANGE, cases.hood(w, h))
            assert (wm_ref <= 1).all() and 0 < int(wm_ref.sum()) < wm_ref.size
            with nmi.NmiLevel(ctx, sc.dx, sc.da, dev(vnp.deep_frame(px, 2, cases.tone_maps()["pct"], RANGE)[0]), S4, WN, 3.0) as base:
                base.set_masks(True, dev(twin_mask))
                assert base.run(mvps, Ms) == ref and (bits(base.outputs()[2]) == bits(t_ref)).all()
            got = []
            for rank in range(2):
                so, sc_, wo, wc = sharding.grid_shard(S4, WN, rank, 2)
                with level(sc_, wc, block=(so, S4, wo, WN)) as blk:
                    got.append(blk.run(mvps[so:so + sc_], Ms[wo:wo + wc]))
                    assert (bits(blk.outputs()[2]) == bits(t_ref[wo:wo + wc, so:so + sc_])).all()
                    assert (blk.masks()[0] == wm_ref[wo:wo + wc]).all()
            assert compose(got) == ref
            with level(0, WN, block=(S4, S4, 0, WN)) as empty, level(S4, WN, block=(0, S4, 0, WN)) as whole:
                assert empty.run(mvps[:0], Ms) == (-1, np.float32(0))
                comm = ctx.rccl_comm_init(capi.rccl_unique_id(), 0, 1)
                try:
                    assert empty.run_rccl(mvps[:0], Ms, comm) == (-1, np.float32(0))
                    assert whole.run_rccl(mvps, Ms, comm) == ref
                    assert (bits(whole.outputs()[2]) == bits(t_ref)).all()
                finally:
                    capi.rccl_comm_destroy(comm)
