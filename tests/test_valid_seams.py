"""GPU tests (-m gpu) of the valid-range kernels past one block column and past one trip of the histogram loops
(the <true> instantiations of nmi_tone.hip and nmi_clahe.hip; include/nmi_hip.h "Deep frames"), == the numpy twin (tests/helpers/valid_np.py) byte for
byte and count for count:
  * every entry of tests/test_valid_frame.py's sweep at contexts 264 x 8 (whole quads) and 261 x 9 (the last quad one pixel, byte
    stores): two block columns of nmi_gray16_kernel<F, true> and nmi_clahe_gray16_kernel<F, true> at F = 1 .. 4, on frames with
    invalid pixels on both sides of output column 256 -- among them seam_pixels, one invalid source pixel under each of the
    output pixels 255, 256 and W - 1;
  * a source of 2104 x 2012 (factor 4) and one of 2101 x 2011 (factor 1): a second chunk of nmi_tone_hist_kernel<false> and
    <true>, a ragged second trip of every tile's workgroups in nmi_clahe_hist_kernel<false> and <true>, on late_quarters frames whose second-trip pixels alone reach the top quarter of 16 bits.
tests/test_intake_geometry.py proves these premises on the CPU."""
import numpy as np
import pytest

from helpers import clahe_np as cnp
from helpers import intake_geometry as geo
from helpers import seam_cases as cases
from helpers import tone_np as tnp
from helpers import valid_cases
from helpers import valid_np as vnp
from orbslam2_nmi_amd import capi
from test_valid_frame import dev, every_entry_equals_the_twin, fresh, same

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def nmi():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    import orbslam2_nmi_amd as m
    m.load_library()
    return m


@pytest.mark.parametrize("size", cases.VALID_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", cases.VALID_FRAMES)
def test_every_entry_equals_the_twin_across_the_block_seam(nmi, name, size):
    every_entry_equals_the_twin(nmi, name, size, valid_cases.FACTORS, frame=cases.valid_frame)


@pytest.mark.parametrize("size", cases.VALID_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_seam_pixels_zeroes_three_pixels_of_the_mask(nmi, size):
    """The mask of seam_pixels in absolute terms: 0 at (255, y0), (256, y1) and (W - 1, y2), 1 everywhere else, under a fixed and
    a tiled tone map."""
    w, h = size
    with nmi.NmiContext(w, h) as ctx:
        for f in valid_cases.FACTORS:
            px, rng, bits, zeros = vnp.seam_pixels(f * w, f * h, f, cases.seam_columns(w), seed=1)
            want = np.ones((h, w), np.uint8)
            for x, y in zeros:
                want[y, x] = 0
            ctx.set_valid_range(*rng)
            for tm in (tnp.tone(tnp.SHIFT, bits), cnp.clahe(8, 8, 1, bits)):
                ctx.set_tone_map(valid_cases.capi_tone(capi, tm))
                _, m = ctx.deep_frame(dev(tnp.pack16(px)), f, out=fresh(h, w), out_mask=fresh(h, w))
                same(m, want, (size, f, tm["mode"]))


def both_ranges():
    return (("off", vnp.OFF), ("on", cases.LATE_RANGE))


@pytest.mark.parametrize("bits", [16, 14])
@pytest.mark.parametrize("run", list(cases.SECOND_TRIP_RUNS))
def test_a_second_chunk_of_the_tone_histograms(nmi, run, bits):
    """nmi_tone_lut under EQUALIZE and PERCENTILE: the table and the window, with the range off (nmi_tone_hist_kernel) and on
    (nmi_tone_hist_kernel<true>), each call twice -- the second on the histogram the first left."""
    w, h, f = cases.SECOND_TRIP_RUNS[run]
    px = cases.second_trip_frame(run, "tone")
    d = dev(tnp.pack16(px))
    with nmi.NmiContext(w, h) as ctx:
        for label, rng in both_ranges():
            ctx.set_valid_range(*rng)
            hist = vnp.histogram(px, bits, rng)
            for tm in (tnp.tone(tnp.EQUALIZE, bits), tnp.tone(tnp.PERCENTILE, bits, p_lo=100, p_hi=100)):
                ctx.set_tone_map(tnp.capi_tone(capi, tm))
                want_lut, want_pair = vnp.table_of_histogram(tm, hist)
                for again in (False, True):
                    lut, pair = ctx.tone_lut(d, f)
                    what = (run, bits, label, tm["mode"], again)
                    assert tuple(pair) == tuple(int(x) for x in want_pair), what
                    same(lut, want_lut, what)


@pytest.mark.parametrize("bits", [16, 14])
@pytest.mark.parametrize("run", list(cases.SECOND_TRIP_RUNS))
def test_a_second_trip_of_every_tile_under_the_range(nmi, run, bits):
    """nmi_tone_tile_luts, tables and counts, with the range on (nmi_clahe_hist_kernel<true>), twice.  (The range off:
    tests/test_clahe_tables.py.)"""
    w, h, f = cases.SECOND_TRIP_RUNS[run]
    px = cases.second_trip_frame(run, "clahe")
    tm = cnp.clahe(*cases.SECOND_TRIP_GRID, 2, bits)
    d = dev(tnp.pack16(px))
    want_luts, want_n = vnp.tile_luts(px, tm, cases.LATE_RANGE)
    assert (want_n < geo.clahe_tile_pixels(*cases.SECOND_TRIP_GRID, f * w, f * h)).all()   # every tile holds an invalid pixel
    with nmi.NmiContext(w, h) as ctx:
        ctx.set_tone_map(cnp.capi_tone(capi, tm))
        ctx.set_valid_range(*cases.LATE_RANGE)
        for again in (False, True):
            luts, n = ctx.tone_tile_luts(d, f)
            assert (n == want_n).all(), (run, bits, again, n, want_n)
            same(luts, want_luts, (run, bits, again))


@pytest.mark.parametrize("label,rng", both_ranges(), ids=[label for label, _ in both_ranges()])
@pytest.mark.parametrize("kernel", ["tone", "clahe"])
def test_deep_frame_on_a_second_trip(nmi, kernel, label, rng):
    """nmi_deep_frame at factor 4 of the 2104 x 2012 source, twice: the statistics of two trips, then three block columns of the
    F = 4 masked conversion."""
    w, h, f = cases.SECOND_TRIP_RUNS["f4"]
    px = cases.second_trip_frame("f4", kernel)
    tm = tnp.tone(tnp.EQUALIZE, 16) if kernel == "tone" else cnp.clahe(*cases.SECOND_TRIP_GRID, 2, 16)
    d = dev(tnp.pack16(px))
    want_gray, want_mask = vnp.deep_frame(px, f, tm, rng)
    assert vnp.is_on(rng) == bool((want_mask == 0).any())
    with nmi.NmiContext(w, h) as ctx:
        ctx.set_tone_map(valid_cases.capi_tone(capi, tm))
        ctx.set_valid_range(*rng)
        for again in (False, True):
            g, m = ctx.deep_frame(d, f, out=fresh(h, w), out_mask=fresh(h, w))
            same(g, want_gray, (kernel, label, again))
            same(m, want_mask, (kernel, label, again, "mask"))
