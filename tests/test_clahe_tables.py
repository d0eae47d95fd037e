"""GPU tests (-m gpu) of the CLAHE tile tables (NMI_TONE_CLAHE, nmi_tone_tile_luts; include/nmi_hip.h "Deep frames"): every
tile's table and pixel count == the numpy model (tests/helpers/clahe_np.py) byte for byte, over the grids, depths, contents and
plateaus of tests/helpers/clahe_cases.py, whose premises tests/test_clahe_model.py asserts on the CPU."""
import ctypes as C

import numpy as np
import pytest

from helpers import clahe_cases as cases
from helpers import clahe_np as cnp
from helpers import seam_cases as seams
from helpers import tone_np as tnp
from orbslam2_nmi_amd import capi

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

E = capi.ERR_INVALID_ARGUMENT


@pytest.fixture(scope="module")
def nmi():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    import orbslam2_nmi_amd as m
    m.load_library()
    return m


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def check_tables(ctx, px, tm, pitch=0, off=0, factor=1):
    """nmi_tone_tile_luts of px under tm == the model: tables and counts; twice, the second run on the histograms the first left."""
    ctx.set_tone_map(cnp.capi_tone(capi, tm))
    want, want_n = cnp.tile_luts(px, tm)
    d = dev(tnp.pack16(px, pitch, off, seed=off + 3))
    for again in (False, True):
        luts, n = ctx.tone_tile_luts(d[off:], factor, pitch)
        got = luts.cpu().numpy()
        assert got.shape == want.shape
        assert (n == want_n).all(), (again, n, want_n)
        assert (got == want).all(), (again, tm, np.argwhere(got != want)[:5])


def test_the_ids_are_the_headers():
    assert capi.TONE_CLAHE == cnp.CLAHE == 6 and capi.TONE_MAX_TILES == 8
    tm = capi.ToneMap.clahe(3, 2, plateau=4, bits=12)
    assert (tm.mode, tm.bits, tm.plateau, tm.tiles_x, tm.tiles_y) == (6, 12, 4, 3, 2)
    assert list(tm.reserved) == [3, 2, 0, 0, 0]                      # the tile counts are the first two former reserved words
    assert "nmi_tone_tile_luts" in capi.EXPORTED_SYMBOLS


@pytest.mark.parametrize("content,bits", [("uniform", 16), ("flat", 16), ("two_valued", 16), ("thermal", 14), ("over_depth", 12),
                                          ("halves", 16)])
@pytest.mark.parametrize("grid", list(cases.GRIDS))
def test_tile_tables_equal_the_model(nmi, grid, content, bits):
    w, h, tx, ty = cases.GRIDS[grid]
    px = cases.content(content, w, h, bits, seed=2)
    with nmi.NmiContext(w, h) as ctx:
        for plateau in (0, 1, 3):
            check_tables(ctx, px, cnp.clahe(tx, ty, plateau, bits))


@pytest.mark.parametrize("bits", [8, 10, 12, 14, 15, 16])
def test_every_depth(nmi, bits):
    """The same 16-bit noise under every depth: values above M saturate into level M; 15 and 16 bits take the histogram's
    two and four passes."""
    w, h, tx, ty = cases.GRIDS["8x8-uneven"]
    px = tnp.uniform(w, h, seed=bits)
    px[::3] >>= 16 - bits                                              # a third of the rows inside the depth
    with nmi.NmiContext(w, h) as ctx:
        for plateau in (0, 2):
            check_tables(ctx, px, cnp.clahe(tx, ty, plateau, bits))
        check_tables(ctx, px, cnp.clahe(3, 2, 1, bits))


@pytest.mark.parametrize("name", list(cases.PLANTED))
def test_planted_plateaus(nmi, name):
    """E, q, r and step on their boundaries in tile (0, 0) (asserted on the model by tests/test_clahe_model.py)."""
    px, tm = cases.planted(name)
    h, w = px.shape
    with nmi.NmiContext(w, h) as ctx:
        check_tables(ctx, px, tm)


def test_a_tile_larger_than_a_workgroups_chunk(nmi):
    """256 x 130 in 2 x 1 tiles: 16,640 pixels a tile, five chunks of 4096 over several workgroups, at 14 bits (one flush behind
    the last chunk) and 16 (a flush per chunk and pass); a flat tile beside a noisy one."""
    w, h = 256, 130
    px = tnp.uniform(w, h, seed=8)
    px[:, :128] = 60000
    with nmi.NmiContext(w, h) as ctx:
        for bits in (14, 16):
            for plateau in (0, 1, 50):
                check_tables(ctx, px, cnp.clahe(2, 1, plateau, bits))
        check_tables(ctx, px, cnp.clahe(1, 1, 7, 16))


@pytest.mark.parametrize("bits", [16, 14])
@pytest.mark.parametrize("run", list(seams.SECOND_TRIP_RUNS))
def test_a_second_trip_of_every_tile(nmi, run, bits):
    """2104 x 2012 (factor 4) and 2101 x 2011 in 8 x 8 tiles: every tile holds more than 16 workgroups x 4096 pixels, so each
    workgroup's stride loop makes a second, ragged trip (tests/test_intake_geometry.py), and only its pixels are in the top
    quarter of 16 bits: `quarters` is reset and read again there; at 14 bits they carry over in the bins to the one flush."""
    w, h, f = seams.SECOND_TRIP_RUNS[run]
    px = seams.second_trip_frame(run, "clahe")
    with nmi.NmiContext(w, h) as ctx:
        check_tables(ctx, px, cnp.clahe(*seams.SECOND_TRIP_GRID, 2, bits), factor=f)


@pytest.mark.parametrize("extra,off", [(2, 0), (10, 2), (64, 6)])
def test_a_pitched_source_with_junk_in_the_padding(nmi, extra, off):
    w, h, tx, ty = cases.GRIDS["8x8-uneven"]
    px = cases.content("thermal", w, h, 14, seed=extra)
    with nmi.NmiContext(w, h) as ctx:
        check_tables(ctx, px, cnp.clahe(tx, ty, 2, 14), pitch=2 * w + extra, off=off)


@pytest.mark.parametrize("factor", [2, 3])
def test_tables_of_a_full_size_source(nmi, factor):
    w, h, tx, ty = cases.REDUCED
    px = cases.content("halves", factor * w, factor * h, 16, seed=factor)
    with nmi.NmiContext(w, h) as ctx:
        check_tables(ctx, px, cnp.clahe(tx, ty, 1, 16), factor=factor)
        check_tables(ctx, px, cnp.clahe(3, 2, 0, 16), pitch=2 * factor * w + 6, factor=factor)


def test_bad_sources_are_refused_and_nothing_is_written(nmi):
    w, h = 64, 48
    src = torch.zeros(w * h * 2 + 4096, dtype=torch.uint8, device="cuda")
    luts = torch.full((2, 3, tnp.LEVELS), 0xAB, dtype=torch.uint8, device="cuda")
    lut = torch.full((tnp.LEVELS,), 0xAB, dtype=torch.uint8, device="cuda")
    counts = (C.c_int32 * 6)(*([-7] * 6))
    pair = (C.c_int32 * 2)(-7, -7)
    sp, lp = src.data_ptr(), luts.data_ptr()
    with nmi.NmiContext(w, h) as ctx:
        lib, hd = ctx._lib, ctx._h
        ctx.set_tone_map(capi.ToneMap.clahe(3, 2, plateau=1, bits=14))
        assert lib.nmi_tone_tile_luts(hd, sp + 1, 0, 1, lp, counts) == E          # an odd base
        assert lib.nmi_tone_tile_luts(hd, sp, 2 * w + 1, 1, lp, counts) == E      # an odd pitch
        assert lib.nmi_tone_tile_luts(hd, sp, 2 * w - 2, 1, lp, counts) == E      # a pitch below the row
        assert lib.nmi_tone_tile_luts(hd, sp, 0, 0, lp, counts) == E
        assert lib.nmi_tone_tile_luts(hd, sp, 0, 5, lp, counts) == E
        assert lib.nmi_tone_tile_luts(hd, None, 0, 1, lp, counts) == E
        assert lib.nmi_tone_tile_luts(hd, sp, 0, 1, None, counts) == E
        assert lib.nmi_tone_tile_luts(None, sp, 0, 1, lp, counts) == E
        assert lib.nmi_tone_tile_luts(hd, sp, 0, 1, sp + 2 * w * h - 1, counts) == E          # the tables meet the source's last byte
        assert lib.nmi_tone_tile_luts(hd, sp + 4096, 0, 1, sp + 4096 - 6 * tnp.LEVELS + 1, counts) == E   # ... and its first
        # no single table under CLAHE, no tile tables under another mode
        assert lib.nmi_tone_lut(hd, sp, 0, 1, lut.data_ptr(), pair) == capi.ERR_UNSUPPORTED
        ctx.set_tone_map(capi.ToneMap.equalize(bits=14))
        assert lib.nmi_tone_tile_luts(hd, sp, 0, 1, lp, counts) == capi.ERR_UNSUPPORTED
        ctx.set_tone_map(None)
        assert lib.nmi_tone_tile_luts(hd, sp, 0, 1, lp, counts) == capi.ERR_UNSUPPORTED
        ctx.synchronize()
    torch.cuda.synchronize()
    assert (luts.cpu().numpy() == 0xAB).all() and (lut.cpu().numpy() == 0xAB).all()
    assert list(counts) == [-7] * 6 and list(pair) == [-7, -7]
