"""GPU tests (-m gpu) of captured levels and keyframe streams fed deep grey frames under NMI_TONE_CLAHE, at 64x48 with S = 3,
Wn = 3 on a small point cloud (as tests/test_tone_pipeline.py).  The baseline is the chain: nmi_gray_frame / nmi_reduce_frame
under the same setting on the context (itself == the model, tests/helpers/clahe_np.py), then the same level or stream on that
8-bit frame as plain grey: the winner, the score's bits, the ratings and the warps must be equal."""
import ctypes as C

import numpy as np
import pytest

from helpers import clahe_np as cnp
from helpers import tone_np as tnp
from helpers import undistort_np as unp
from orbslam2_nmi_amd import capi
from test_clahe_frame import bad_clahe_maps
from test_color_level import bits, lens_K, scene
from test_color_stream import outcome, same
from test_masked_level import dev, views, warps
from test_reduce_level import full_size
from test_stream_masked import level, pin
from test_tone_pipeline import deep

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

W, H, S, WN = 64, 48, 3, 3
BITS = 14
RADTAN = unp.FAMILIES["barrel"]
E = capi.ERR_INVALID_ARGUMENT
# factor, lens
VARIANTS = {"cloud": (1, False), "radtan": (1, True), "f2": (2, False)}


@pytest.fixture(scope="module")
def nmi():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    import orbslam2_nmi_amd as m
    m.load_library()
    return m


def replay(lv, mvps, Ms):
    win = lv.run(mvps, Ms)
    _, ws, t = lv.outputs()
    return win, t.copy(), ws.copy()


def same_replay(a, b):
    assert a[0][0] == b[0][0], (a[0], b[0])
    assert bits(np.float32(a[0][1])) == bits(np.float32(b[0][1])), (a[0], b[0])
    assert (bits(a[1]) == bits(b[1])).all()
    assert (a[2] == b[2]).all()


def chain_frame(ctx, d, f, pitch, tm):
    """The chain's first link: the context's own conversion of the deep frame, which is the model's."""
    ctx.set_tone_map(cnp.capi_tone(capi, tm))
    g = ctx.reduce_frame(d, capi.FRAME_GRAY16, f, pitch) if f > 1 else ctx.gray_frame(d, capi.FRAME_GRAY16, pitch)
    return g


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_a_clahe_level_equals_the_chain(nmi, variant):
    """Two frames in place in the level's frame, two settings (8 x 8 without a plateau, 3 x 2 with one): every replay is the chain's."""
    f, lens = VARIANTS[variant]
    pitch, off = 2 * f * W + 10, 2
    with nmi.NmiContext(W, H) as ctx:
        sc = scene(nmi, ctx, W, H, False, "plain")
        K = lens_K(sc.rp)
        gray0 = sc.frame.cpu().numpy()
        frames = [deep(g if f == 1 else full_size(g, f, 1), "bright", seed=k) for k, g in enumerate((gray0, np.roll(gray0, 7, axis=1)))]
        frames[1][:, :f * W // 2] //= 8                                   # a dark left half: tiles that differ
        d = dev(tnp.pack16(frames[0], pitch, off, seed=2))
        twin_frame = dev(np.zeros((H, W), np.uint8))
        mvps, Ms = views(sc.rp, S), warps(W, H, WN)
        seen = []
        with nmi.NmiLevel(ctx, sc.dx, sc.da, d[off:], S, WN, 3.0) as lv, nmi.NmiLevel(ctx, sc.dx, sc.da, twin_frame, S, WN, 3.0) as base:
            for target in (lv, base):
                if lens:
                    target.set_distortion(K, RADTAN)
            lv.set_frame_reduction(f, capi.FRAME_GRAY16, pitch)
            for tm in (cnp.clahe(8, 8, 0, BITS), cnp.clahe(3, 2, 4, BITS)):
                lv.set_tone_map(cnp.capi_tone(capi, tm))
                for k in (0, 1, 0):
                    buf = tnp.pack16(frames[k], pitch, off, seed=2 + k)
                    d.copy_(dev(buf))
                    g = chain_frame(ctx, d[off:], f, pitch, tm)
                    assert (g.cpu().numpy() == cnp.reduce_frame(buf, W, H, f, tm, pitch, off)).all()
                    twin_frame.copy_(g)
                    torch.cuda.synchronize()
                    got = replay(lv, mvps, Ms)
                    same_replay(got, replay(base, mvps, Ms))
                    seen.append(bits(got[1]).copy())
            assert (seen[0] != seen[1]).any() and (seen[0] == seen[2]).all() and (seen[0] != seen[3]).any()
            # every bad setting is refused and the level replays as before
            for name, bad in bad_clahe_maps().items():
                if "> W" in name or "> H" in name:
                    continue                                           # (fine on 64 x 48: the small level below)
                assert ctx._lib.nmi_level_set_tone_map(lv._h, C.byref(bad)) == E, name
            same_replay(replay(lv, mvps, Ms), replay(base, mvps, Ms))


def test_a_level_switches_between_clahe_and_equalize(nmi):
    with nmi.NmiContext(W, H) as ctx:
        sc = scene(nmi, ctx, W, H, False, "plain")
        px = deep(sc.frame.cpu().numpy())
        px[:, W // 2:] //= 4
        buf = tnp.pack16(px)
        d = dev(buf)
        twin_frame = dev(np.zeros((H, W), np.uint8))
        mvps, Ms = views(sc.rp, S), warps(W, H, WN)
        with nmi.NmiLevel(ctx, sc.dx, sc.da, d, S, WN, 3.0) as lv, nmi.NmiLevel(ctx, sc.dx, sc.da, twin_frame, S, WN, 3.0) as base:
            lv.set_tone_map(cnp.capi_tone(capi, cnp.clahe(8, 8, 2, BITS)))   # before the format: kept
            lv.set_frame_format(capi.FRAME_GRAY16, 0)
            results = []
            for tm in (cnp.clahe(8, 8, 2, BITS), tnp.tone(tnp.EQUALIZE, BITS), cnp.clahe(8, 8, 2, BITS), cnp.clahe(2, 3, 0, BITS), None):
                tiled = tm is not None and tm["mode"] == cnp.CLAHE
                if results:
                    lv.set_tone_map(None if tm is None else cnp.capi_tone(capi, tm) if tiled else tnp.capi_tone(capi, tm))
                twin = cnp.to_gray(buf, W, H, tm) if tiled else tnp.to_gray(buf, W, H, tm or tnp.tone())
                twin_frame.copy_(dev(twin))
                torch.cuda.synchronize()
                got = replay(lv, mvps, Ms)
                same_replay(got, replay(base, mvps, Ms))
                results.append(bits(got[1]).copy())
            assert (results[0] == results[2]).all() and (results[0] != results[1]).any() and (results[2] != results[3]).any()


def test_a_small_level_refuses_more_tiles_than_pixels(nmi):
    """A 6 x 4 level: tiles_x == W, tiles_y == H is accepted, one more on either axis refused with the setting in force."""
    w, h = 6, 4
    with nmi.NmiContext(w, h) as ctx:
        sc = scene(nmi, ctx, w, h, False, "plain")
        px = tnp.uniform(w, h, seed=3)
        d = dev(tnp.pack16(px))
        mvps, Ms = views(sc.rp, 2), warps(w, h, WN)
        good = cnp.clahe(6, 4, 1, 16)
        twin_frame = dev(cnp.apply(px, good))
        with nmi.NmiLevel(ctx, sc.dx, sc.da, d, 2, WN, 3.0) as lv, nmi.NmiLevel(ctx, sc.dx, sc.da, twin_frame, 2, WN, 3.0) as base:
            lv.set_frame_format(capi.FRAME_GRAY16, 0)
            lv.set_tone_map(cnp.capi_tone(capi, good))
            for name, bad in bad_clahe_maps().items():
                assert ctx._lib.nmi_level_set_tone_map(lv._h, C.byref(bad)) == E, name
            same_replay(replay(lv, mvps, Ms), replay(base, mvps, Ms))


@pytest.mark.parametrize("tiles", [(8, 8, 0), (3, 2, 3)], ids=["8x8", "3x2-plateau"])
def test_clahe_tickets_equal_the_chains_tickets(nmi, tiles):
    tm = cnp.clahe(tiles[0], tiles[1], tiles[2], BITS)
    pitch = 2 * W + 6
    frames = [level(W, H, (3, 1, 1), (3, 1, 1), seed=s) for s in (5, 9)]
    Ms = frames[0][2]
    with nmi.NmiContext(W, H) as ctx, nmi.NmiStream(ctx, S, WN, depth=4) as st, nmi.NmiStream(ctx, S, WN, depth=4) as ref:
        st.keep_ratings()
        ref.keep_ratings()
        st.set_frame_format(capi.FRAME_GRAY16, pitch)
        st.set_tone_map(cnp.capi_tone(capi, tm))
        for name, bad in bad_clahe_maps().items():
            if "> W" not in name and "> H" not in name:
                assert ctx._lib.nmi_stream_set_tone_map(st._h, C.byref(bad)) == E, name
        pairs = []
        for k, (F, rs, _) in enumerate(frames):
            px = deep(F, ("bright", "dark")[k], seed=k)
            px[:, :W // 2] //= 2 + k
            buf = tnp.pack16(px, pitch, seed=k)
            g = chain_frame(ctx, dev(buf), 1, pitch, tm).cpu().numpy()
            assert (g == cnp.to_gray(buf, W, H, tm, pitch)).all()
            t = st.submit(pin(rs), pin(buf), Ms)
            r = ref.submit(pin(rs), pin(g), Ms)
            pairs.append((t, r))
        for t, r in pairs:
            same(outcome(st, t, WN, S, "plain"), outcome(ref, r, WN, S, "plain"))
