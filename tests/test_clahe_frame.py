"""GPU tests (-m gpu) of GRAY16 conversions under NMI_TONE_CLAHE (nmi_gray_frame, nmi_reduce_frame; include/nmi_hip.h "Deep
frames"): the blend of the four nearest tiles' tables per source pixel, then the box average == the numpy model
(tests/helpers/clahe_np.py) byte for byte; what a context keeps between frames and settings; and what the setters refuse."""
import ctypes as C

import numpy as np
import pytest

from helpers import clahe_cases as cases
from helpers import clahe_np as cnp
from helpers import reduce_np as rnp
from helpers import tone_np as tnp
from orbslam2_nmi_amd import capi

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

E = capi.ERR_INVALID_ARGUMENT
G16 = capi.FRAME_GRAY16
C_INT5 = C.c_int32 * 5


@pytest.fixture(scope="module")
def nmi():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    import orbslam2_nmi_amd as m
    m.load_library()
    return m


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def gray(ctx, px, pitch=0, off=0):
    h, w = px.shape
    out = torch.full((h, w), 0xAB, dtype=torch.uint8, device="cuda")
    ctx.gray_frame(dev(tnp.pack16(px, pitch, off, seed=off + 1))[off:], G16, pitch, out=out)
    return out.cpu().numpy()


def same(got, want, what):
    assert (got == want).all(), (what, np.argwhere(got != want)[:5])


@pytest.mark.parametrize("content,bits", [("halves", 16), ("uniform", 16), ("flat", 16), ("thermal", 14), ("over_depth", 12)])
@pytest.mark.parametrize("grid", list(cases.GRIDS))
def test_gray_frame_equals_the_model(nmi, grid, content, bits):
    """Dense and pitched, bases 0, 2 and 6 bytes into the allocation (the vector and the 2-byte loads), plateaus 0 and 2."""
    w, h, tx, ty = cases.GRIDS[grid]
    px = cases.content(content, w, h, bits, seed=4)
    with nmi.NmiContext(w, h) as ctx:
        for plateau in (0, 2):
            tm = cnp.clahe(tx, ty, plateau, bits)
            ctx.set_tone_map(cnp.capi_tone(capi, tm))
            want = cnp.apply(px, tm)
            for pitch, off in ((0, 0), (2 * w + 2, 2), (2 * w + 64, 6), (2 * w + 16, 0)):
                same(gray(ctx, px, pitch, off), want, (plateau, pitch, off))


@pytest.mark.parametrize("grid", ["8x8", "3x2", "8x8-uneven"])
def test_the_half_tiles_at_the_edges_and_a_frame_whose_tiles_differ(nmi, grid):
    """Left half near 1000, right half near 40000 (and top / bottom likewise): the tables of neighbouring tiles differ, so a
    wrong weight or neighbour shows; the first and last half tile of both axes take their own tile's table alone."""
    w, h, tx, ty = cases.GRIDS[grid]
    for px in (cnp.halves(w, h, seed=1), cnp.halves(h, w, seed=2).T.copy()):
        tm = cnp.clahe(tx, ty, 0, 16)
        luts, _ = cnp.tile_luts(px, tm)
        want = cnp.apply(px, tm)
        assert (want != cnp.apply(px, cnp.clahe(1, 1, 0, 16))).any()
        with nmi.NmiContext(w, h) as ctx:
            ctx.set_tone_map(cnp.capi_tone(capi, tm))
            got = gray(ctx, px)
        same(got, want, grid)
        edge_x, edge_y = w // (2 * tx), h // (2 * ty)                  # whole columns / rows inside the first half tile
        v = np.asarray(px, np.int64)
        assert (got[:edge_y, :edge_x] == luts[0, 0][v[:edge_y, :edge_x]]).all()
        assert (got[h - edge_y:, w - edge_x:] == luts[ty - 1, tx - 1][v[h - edge_y:, w - edge_x:]]).all()
        assert (got[:edge_y, w - edge_x:] == luts[0, tx - 1][v[:edge_y, w - edge_x:]]).all()


@pytest.mark.parametrize("factor", cases.FACTORS)
@pytest.mark.parametrize("tiles", [(8, 8), (3, 2)], ids=["8x8", "3x2"])
def test_reduce_frame_equals_the_model(nmi, factor, tiles):
    """Statistics, tiles and blend on the full-size source, then the box average; with a source mask the mask is the existing
    rule's and the grey frame is unchanged.  Factors 3 and 4 under the 8 x 8 grid also at a context of 264 x 8: a second block
    column of the conversion."""
    reduce_frame_equals_the_model(nmi, cases.REDUCED[:2], factor, tiles)
    if factor >= 3 and tiles == (8, 8):
        reduce_frame_equals_the_model(nmi, (264, 8), factor, tiles)


def reduce_frame_equals_the_model(nmi, size, factor, tiles):
    w, h = size
    tx, ty = tiles
    sw, sh = factor * w, factor * h
    mask = (np.random.default_rng(7).random((sh, sw)) < 0.9).astype(np.uint8) * 3
    with nmi.NmiContext(w, h) as ctx:
        for content, bits, plateau in (("halves", 16, 0), ("thermal", 14, 2), ("uniform", 16, 1)):
            px = cases.content(content, sw, sh, bits, seed=factor)
            tm = cnp.clahe(tx, ty, plateau, bits)
            ctx.set_tone_map(cnp.capi_tone(capi, tm))
            for pitch, off in ((0, 0), (2 * sw + 10, 2)):
                buf = tnp.pack16(px, pitch, off, seed=5)
                want = cnp.reduce_frame(buf, w, h, factor, tm, pitch, off)
                d = dev(buf)
                out = torch.full((h, w), 0xAB, dtype=torch.uint8, device="cuda")
                ctx.reduce_frame(d[off:], G16, factor, pitch, out=out)
                same(out.cpu().numpy(), want, (content, pitch))
                g2, m2 = ctx.reduce_frame(d[off:], G16, factor, pitch, src_mask=dev(mask))
                same(g2.cpu().numpy(), want, (content, pitch, "masked"))
                assert (m2.cpu().numpy() == rnp.reduce_mask(mask, factor)).all()
            if factor == 1:
                same(gray(ctx, px), want, content)


@pytest.mark.parametrize("w", [(1 << 19) - 4, 1 << 19], ids=["below-2^19", "2^19"])
def test_a_very_wide_frame(nmi, w):
    """The weights' one quotient (256 ((2x+1) tiles + Ws)) / (2 Ws) is taken in 32 bits while 4352 Ws fits them, in 64 from
    Ws = 2^19 on: the widest frame of the first kind and the narrowest of the second, 8 rows, 8 x 8 tiles of one row each."""
    h = 8
    rng = np.random.default_rng(w & 7)
    px = (rng.integers(0, 256, (h, w)) + (np.arange(w)[None, :] * 3840 // w)).astype(np.uint16)   # a ramp over 12 bits, with noise
    tm = cnp.clahe(8, 8, 3, 12)
    want = cnp.apply(px, tm)
    with nmi.NmiContext(w, h) as ctx:
        ctx.set_tone_map(cnp.capi_tone(capi, tm))
        same(gray(ctx, px), want, w)


def test_every_frame_gets_its_own_statistics(nmi):
    """Two different frames back to back, then the first again: the tile histograms were left zero."""
    w, h, tx, ty = cases.GRIDS["8x8-uneven"]
    a, b = cases.content("thermal", w, h, 14, seed=1), cases.content("halves", w, h, 14, seed=2)
    tm = cnp.clahe(tx, ty, 3, 14)
    with nmi.NmiContext(w, h) as ctx:
        ctx.set_tone_map(cnp.capi_tone(capi, tm))
        for px in (a, b, a, a):
            same(gray(ctx, px), cnp.apply(px, tm), "back to back")
        luts, n = ctx.tone_tile_luts(dev(tnp.pack16(b)))
        want, want_n = cnp.tile_luts(b, tm)
        assert (n == want_n).all() and (luts.cpu().numpy() == want).all()
        same(gray(ctx, a), cnp.apply(a, tm), "after the tables")


def test_a_context_follows_its_setting(nmi):
    """CLAHE -> EQUALIZE -> CLAHE, 8 x 8 -> 3 x 2 -> 1 x 1 -> 8 x 8, 16 bits -> 10 -> 16: each conversion is the model's for the
    setting in force."""
    w, h = 64, 48
    px = cases.content("halves", w, h, 16, seed=3)
    steps = [cnp.clahe(8, 8, 0, 16), tnp.tone(tnp.EQUALIZE, 16), cnp.clahe(8, 8, 0, 16), cnp.clahe(3, 2, 2, 16), cnp.clahe(1, 1, 1, 10),
             tnp.tone(tnp.PERCENTILE, 16, p_lo=100, p_hi=100), cnp.clahe(8, 8, 1, 16), tnp.tone(tnp.SHIFT, 16), cnp.clahe(2, 8, 0, 12)]
    with nmi.NmiContext(w, h) as ctx:
        seen = []
        for tm in steps:
            tiled = tm["mode"] == cnp.CLAHE
            ctx.set_tone_map(cnp.capi_tone(capi, tm) if tiled else tnp.capi_tone(capi, tm))
            want = cnp.apply(px, tm) if tiled else tnp.apply(px, tm)
            got = gray(ctx, px)
            same(got, want, tm)
            seen.append(got)
        assert (seen[0] == seen[2]).all() and (seen[0] != seen[1]).any() and (seen[2] != seen[3]).any()


def bad_clahe_maps():
    T = capi.ToneMap
    return {
        "tiles_x 0": T.clahe(0, 8), "tiles_y 0": T.clahe(8, 0), "tiles_x 9": T.clahe(9, 8), "tiles_y 9": T.clahe(8, 9),
        "tiles_x -1": T.clahe(-1, 8), "tiles_y -3": T.clahe(8, -3), "no tiles": T(mode=capi.TONE_CLAHE, bits=16),
        "tiles_x > W": T.clahe(7, 2), "tiles_y > H": T.clahe(2, 5),       # (the context below is 6 x 4)
        "plateau < 0": T.clahe(2, 2, plateau=-1), "bits 7": T.clahe(2, 2, bits=7), "bits 17": T.clahe(2, 2, bits=17),
        "reserved third": T(mode=capi.TONE_CLAHE, bits=16, reserved=C_INT5(2, 2, 1, 0, 0)),
        "reserved last": T(mode=capi.TONE_CLAHE, bits=16, reserved=C_INT5(2, 2, 0, 0, 9)),
        "mode 5": T(mode=5, bits=16, reserved=C_INT5(2, 2, 0, 0, 0)), "mode 7": T(mode=7, bits=16, reserved=C_INT5(2, 2, 0, 0, 0)),
        "equalize with tiles": T(mode=capi.TONE_EQUALIZE, bits=16, reserved=C_INT5(0, 2, 0, 0, 0)),
    }


def test_bad_settings_leave_the_setting(nmi):
    """On a 6 x 4 context (and a stream of it; levels and streams in force: tests/test_clahe_pipeline.py):
    NMI_ERR_INVALID_ARGUMENT, and the earlier CLAHE setting converts as before."""
    w, h = 6, 4
    px = tnp.uniform(w, h, seed=9)
    good = cnp.clahe(6, 4, 1, 16)                                      # tiles_x == W, tiles_y == H: accepted
    want = cnp.apply(px, good)
    with nmi.NmiContext(w, h) as ctx, nmi.NmiStream(ctx, 2, 2) as st:
        ctx.set_tone_map(cnp.capi_tone(capi, good))
        st.set_tone_map(cnp.capi_tone(capi, good))
        for name, tm in bad_clahe_maps().items():
            assert ctx._lib.nmi_set_tone_map(ctx._h, C.byref(tm)) == E, name
            assert ctx._lib.nmi_stream_set_tone_map(st._h, C.byref(tm)) == E, name
            assert ctx._lib.nmi_level_set_tone_map(None, C.byref(tm)) == E, name
        same(gray(ctx, px), want, "the setting is the good one still")
