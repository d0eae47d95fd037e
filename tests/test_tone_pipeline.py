"""GPU tests (-m gpu) of captured levels and keyframe streams fed deep grey frames (NMI_FRAME_GRAY16 with a tone map, through
nmi_level_set_frame_format / _set_frame_reduction / _set_tone_map and their nmi_stream_* twins), at 64x48 with S = 3, Wn = 3 on a
small point cloud.  The baseline is always the same pipeline given the numpy twin's 8-bit frame (tests/helpers/tone_np.py) as
plain grey: the winner, the score's bits and the rating table must be equal."""
import numpy as np
import pytest

from helpers import tone_np as tnp
from helpers import undistort_np as unp
from orbslam2_nmi_amd import capi
from test_color_level import bits, enable, lens_K, scene
from test_color_stream import outcome, same
from test_masked_level import dev, hood_mask, views, warps
from test_reduce_level import full_size
from test_stream_masked import level, pin

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

W, H, S, WN = 64, 48, 3, 3
BITS = 14
RADTAN = unp.FAMILIES["barrel"]
# factor, lens, masks
VARIANTS = {"plain": (1, False, False), "f2": (2, False, False), "radtan": (1, True, False), "masked": (1, False, True),
            "f2-radtan-masked": (2, True, True)}


@pytest.fixture(scope="module")
def nmi():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    import orbslam2_nmi_amd as m
    m.load_library()
    return m


def deep(gray, band="bright", seed=0):
    """An 8-bit frame as a 14-bit one: a band of a few hundred counts (bright: around 9000, dark: around 300), or flat."""
    g = np.asarray(gray, np.int64)
    if band == "flat":
        return np.full(g.shape, 5000, np.uint16)
    noise = np.random.default_rng(seed).integers(0, 3, g.shape)
    return ((9000 if band == "bright" else 300) + 3 * g + noise).astype(np.uint16)


def tone_maps(lut=None):
    return {"shift": tnp.tone(tnp.SHIFT, BITS), "window": tnp.tone(tnp.WINDOW, BITS, lo=9100, hi=9700),
            "pct": tnp.tone(tnp.PERCENTILE, BITS, p_lo=100, p_hi=100), "equalize": tnp.tone(tnp.EQUALIZE, BITS),
            "table": tnp.tone(tnp.TABLE, BITS, lut=lut)}


def replay(lv, mvps, Ms):
    win = lv.run(mvps, Ms)
    return win, lv.outputs()[2].copy()


def same_replay(a, b):
    assert a[0][0] == b[0][0], (a[0], b[0])
    assert bits(np.float32(a[0][1])) == bits(np.float32(b[0][1])), (a[0], b[0])
    assert (bits(a[1]) == bits(b[1])).all()


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_deep_level_equals_the_level_on_the_twins_frame(nmi, variant):
    f, lens, masked = VARIANTS[variant]
    pitch, off = 2 * f * W + 10, 2
    with nmi.NmiContext(W, H) as ctx:
        sc = scene(nmi, ctx, W, H, False, "masked" if masked else "plain")
        K = lens_K(sc.rp)
        gray0 = sc.frame.cpu().numpy()
        px = deep(gray0 if f == 1 else full_size(gray0, f, 1))
        buf = tnp.pack16(px, pitch, off, seed=2)
        d = dev(buf)
        fm = dev(hood_mask(W, H)) if masked else None
        mvps, Ms = views(sc.rp, S), warps(W, H, WN)
        table = np.random.default_rng(3).integers(0, 256, tnp.LEVELS).astype(np.uint8)
        table[9000:9800] = np.sort(table[9000:9800])               # (any table will do; this one keeps the scene recognisable)
        d_table = dev(table)
        twin_frame = dev(np.zeros((H, W), np.uint8))
        seen = []
        with nmi.NmiLevel(ctx, sc.dx, sc.da, d[off:], S, WN, 3.0) as lv, nmi.NmiLevel(ctx, sc.dx, sc.da, twin_frame, S, WN, 3.0) as base:
            for target in (lv, base):
                if lens:
                    target.set_distortion(K, RADTAN)
                enable(target, "masked" if masked else "plain", fm)
            lv.set_frame_reduction(f, capi.FRAME_GRAY16, pitch)
            for name, tm in tone_maps(table).items():
                lv.set_tone_map(tnp.capi_tone(capi, tm, d_table))
                twin_frame.copy_(dev(tnp.reduce_frame(buf, W, H, f, tm, pitch, off)))
                torch.cuda.synchronize()
                got, want = replay(lv, mvps, Ms), replay(base, mvps, Ms)
                same_replay(got, want)
                seen.append(bits(got[1]).copy())
            assert (seen[0] != seen[3]).any()                      # SHIFT and EQUALIZE are different frames
            for bad in (capi.ToneMap(mode=5, bits=14), capi.ToneMap(mode=capi.TONE_WINDOW, bits=14, lo=5, hi=5),
                        capi.ToneMap(mode=capi.TONE_SHIFT, bits=17), capi.ToneMap(mode=capi.TONE_TABLE, bits=14)):
                with pytest.raises(capi.NmiError):
                    lv.set_tone_map(bad)
            same_replay(replay(lv, mvps, Ms), want)                # as it was: the TABLE setting


@pytest.mark.parametrize("mode", ["pct", "equalize"])
def test_statistics_start_clean_at_every_replay(nmi, mode):
    """Bright band, dark band, flat, bright again, in place in the level's frame: each replay is the twin's for that frame."""
    pitch = 2 * W
    tm = tone_maps()[mode]
    with nmi.NmiContext(W, H) as ctx:
        sc = scene(nmi, ctx, W, H, False, "plain")
        gray0 = sc.frame.cpu().numpy()
        d = dev(tnp.pack16(deep(gray0)))
        twin_frame = dev(np.zeros((H, W), np.uint8))
        mvps, Ms = views(sc.rp, S), warps(W, H, WN)
        with nmi.NmiLevel(ctx, sc.dx, sc.da, d, S, WN, 3.0) as lv, nmi.NmiLevel(ctx, sc.dx, sc.da, twin_frame, S, WN, 3.0) as base:
            lv.set_frame_format(capi.FRAME_GRAY16, pitch)
            lv.set_tone_map(tnp.capi_tone(capi, tm))
            tables = []
            for k, band in enumerate(("bright", "dark", "flat", "bright")):
                buf = tnp.pack16(deep(np.roll(gray0, k, axis=1), band, seed=k))
                d.copy_(dev(buf))
                twin = tnp.to_gray(buf, W, H, tm)
                twin_frame.copy_(dev(twin))
                torch.cuda.synchronize()
                got = replay(lv, mvps, Ms)
                same_replay(got, replay(base, mvps, Ms))
                tables.append(bits(got[1]).copy())
                if band == "flat":
                    assert (twin == 0).all()
            assert (tables[0] != tables[2]).any()


def test_a_level_follows_its_tone_map_setting(nmi):
    """EQUALIZE -> WINDOW -> EQUALIZE -> the default: each replay equals the twin's for the setting then in force."""
    with nmi.NmiContext(W, H) as ctx:
        sc = scene(nmi, ctx, W, H, False, "plain")
        buf = tnp.pack16(deep(sc.frame.cpu().numpy()))
        d = dev(buf)
        twin_frame = dev(np.zeros((H, W), np.uint8))
        mvps, Ms = views(sc.rp, S), warps(W, H, WN)
        maps = tone_maps()
        with nmi.NmiLevel(ctx, sc.dx, sc.da, d, S, WN, 3.0) as lv, nmi.NmiLevel(ctx, sc.dx, sc.da, twin_frame, S, WN, 3.0) as base:
            lv.set_tone_map(tnp.capi_tone(capi, maps["equalize"]))   # before the format: kept
            lv.set_frame_format(capi.FRAME_GRAY16, 0)
            results = []
            for tm in (maps["equalize"], maps["window"], maps["equalize"], None):
                if results:
                    lv.set_tone_map(None if tm is None else tnp.capi_tone(capi, tm))
                twin_frame.copy_(dev(tnp.to_gray(buf, W, H, tm or tnp.tone())))
                torch.cuda.synchronize()
                got = replay(lv, mvps, Ms)
                same_replay(got, replay(base, mvps, Ms))
                results.append(bits(got[1]).copy())
            assert (results[0] == results[2]).all() and (results[0] != results[1]).any()


@pytest.mark.parametrize("mode", ["shift", "pct", "equalize"])
def test_deep_tickets_equal_grey_tickets(nmi, mode):
    tm = tone_maps()[mode]
    pitch = 2 * W + 6
    frames = [level(W, H, (3, 1, 1), (3, 1, 1), seed=s) for s in (5, 9, 11)]
    Ms = frames[0][2]
    with nmi.NmiContext(W, H) as ctx, nmi.NmiStream(ctx, S, WN, depth=4) as st, nmi.NmiStream(ctx, S, WN, depth=4) as ref:
        st.keep_ratings()
        ref.keep_ratings()
        st.set_frame_format(capi.FRAME_GRAY16, pitch)
        st.set_tone_map(tnp.capi_tone(capi, tm))
        with pytest.raises(capi.NmiError):
            st.set_tone_map(capi.ToneMap(mode=capi.TONE_PERCENTILE, bits=14, p_lo=5000, p_hi=5000))
        pairs = []
        for k, (F, rs, _) in enumerate(frames):
            band = ("bright", "dark", "flat")[k]
            buf = tnp.pack16(deep(F, band, seed=k), pitch, seed=k)
            t = st.submit(pin(rs), pin(buf), Ms)
            r = ref.submit(pin(rs), pin(tnp.to_gray(buf, W, H, tm, pitch)), Ms)
            pairs.append((t, r))
        for t, r in pairs:
            same(outcome(st, t, WN, S, "plain"), outcome(ref, r, WN, S, "plain"))


def test_a_table_from_one_frame_maps_another(nmi):
    with nmi.NmiContext(W, H) as ctx:
        sc = scene(nmi, ctx, W, H, False, "plain")
        gray0 = sc.frame.cpu().numpy()
        buf_a, buf_b = tnp.pack16(deep(gray0, "bright", 1)), tnp.pack16(deep(np.roll(gray0, 5, axis=1), "bright", 2) + 40)
        d_a, d_b = dev(buf_a), dev(buf_b)
        eq = tone_maps()["equalize"]
        ctx.set_tone_map(tnp.capi_tone(capi, eq))
        lut, pair = ctx.tone_lut(d_a)
        want_lut, want_pair = tnp.lut_of(buf_a, W, H, eq)
        assert pair == want_pair and (lut.cpu().numpy() == want_lut).all()
        held = tnp.tone(tnp.TABLE, BITS, lut=want_lut)
        twin = tnp.to_gray(buf_b, W, H, held)
        assert (twin != tnp.to_gray(buf_b, W, H, eq)).any()           # B's own equalisation is another frame
        ctx.set_tone_map(capi.ToneMap.from_table(lut, BITS))
        assert (ctx.gray_frame(d_b, capi.FRAME_GRAY16).cpu().numpy() == twin).all()
        mvps, Ms = views(sc.rp, S), warps(W, H, WN)
        with nmi.NmiLevel(ctx, sc.dx, sc.da, d_b, S, WN, 3.0) as lv, nmi.NmiLevel(ctx, sc.dx, sc.da, dev(twin), S, WN, 3.0) as base:
            lv.set_frame_format(capi.FRAME_GRAY16, 0)
            lv.set_tone_map(capi.ToneMap.from_table(lut, BITS))
            same_replay(replay(lv, mvps, Ms), replay(base, mvps, Ms))
