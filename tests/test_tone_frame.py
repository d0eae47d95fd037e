"""GPU tests (-m gpu) of nmi_gray_frame and nmi_tone_lut on deep grey frames (NMI_FRAME_GRAY16, include/nmi_hip.h "Deep
frames"): all five tone modes == the numpy twin (tests/helpers/tone_np.py), from 1x1 up, dense and pitched rows, source bases 0,
2 and 6 bytes into their allocation, on contents from noise to a flat frame, and with one value planted at the counts where a
16-bit counter would wrap."""
import numpy as np
import pytest

from helpers import tone_np as tnp
from orbslam2_nmi_amd import capi

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

# 1x1: one pixel is the whole statistic; 2x2, 5x3: ragged quads and runs only; 64x48: whole quads and runs on the vector paths;
# 1241x376: an odd width, many workgroups; 256x257: 65,792 pixels, room for one value 65,537 times
SHAPES = [(1, 1), (2, 2), (5, 3), (64, 48), (1241, 376), (256, 257)]
# content -> (pixels, bits).  uniform15: the two-pass histogram; the others at 16 bits take one to four passes by content
CONTENTS = {
    "uniform": (lambda w, h: tnp.uniform(w, h, 1), 16),
    "uniform15": (lambda w, h: tnp.uniform(w, h, 2), 15),
    "flat": (lambda w, h: tnp.flat(w, h), 16),
    "two": (lambda w, h: tnp.two_valued(w, h), 16),
    "thermal": (lambda w, h: tnp.thermal(w, h, 3), 14),
    "over12": (lambda w, h: tnp.over_depth(w, h, 4), 12),
}
PLANTED = (65535, 65536, 65537)


@pytest.fixture(scope="module")
def nmi():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    import orbslam2_nmi_amd as m
    m.load_library()
    return m


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def tones(bits, seed=0):
    m = (1 << bits) - 1
    lut = np.random.default_rng(seed).integers(0, 256, tnp.LEVELS).astype(np.uint8)   # (not saturated above M: the kernel clamps)
    return {"shift": tnp.tone(tnp.SHIFT, bits), "window": tnp.tone(tnp.WINDOW, bits, lo=m // 9, hi=m - m // 5),
            "minmax": tnp.tone(tnp.PERCENTILE, bits), "pct": tnp.tone(tnp.PERCENTILE, bits, p_lo=100, p_hi=100),
            "equalize": tnp.tone(tnp.EQUALIZE, bits), "plateau": tnp.tone(tnp.EQUALIZE, bits, plateau=2),
            "table": tnp.tone(tnp.TABLE, bits, lut=lut)}


def check_frame(ctx, px, bits, layouts):
    """Every tone mode on the pixels px, in every layout: the grey frame, the table and the window pair == the twin's."""
    h, w = px.shape
    for name, tm in tones(bits).items():
        d_lut = dev(tm["lut"]) if tm["mode"] == tnp.TABLE else None
        ctx.set_tone_map(tnp.capi_tone(capi, tm, d_lut))
        want = tnp.apply(px, tm)                                   # (the statistics do not depend on the layout)
        want_lut, want_pair = tnp.table(tm, tnp.histogram(px, bits))
        for extra, off in layouts:
            pitch = 0 if extra is None else 2 * w + extra
            buf = tnp.pack16(px, pitch, off, seed=off + 1)
            d = dev(buf)
            out = torch.full((h, w), 0xAB, dtype=torch.uint8, device="cuda")
            ctx.gray_frame(d[off:], capi.FRAME_GRAY16, pitch, out=out)
            got = out.cpu().numpy()
            assert (got == want).all(), (name, pitch, off, np.argwhere(got != want)[:5])
            lut, pair = ctx.tone_lut(d[off:], 1, pitch)
            assert pair == want_pair, (name, pitch, off, pair, want_pair)
            assert (lut.cpu().numpy() == want_lut).all(), (name, pitch, off)
            again = ctx.gray_frame(d[off:], capi.FRAME_GRAY16, pitch)   # the histogram was left clean
            assert (again.cpu().numpy() == want).all(), (name, pitch, off)


def test_the_ids_are_the_headers():
    assert capi.FRAME_GRAY16 == tnp.GRAY16 == 48 and capi.FRAME_BYTES_PER_PIXEL[48] == 2
    assert (capi.TONE_SHIFT, capi.TONE_WINDOW, capi.TONE_PERCENTILE, capi.TONE_EQUALIZE, capi.TONE_TABLE) == (0, 1, 2, 3, 4)
    assert (tnp.SHIFT, tnp.WINDOW, tnp.PERCENTILE, tnp.EQUALIZE, tnp.TABLE) == (0, 1, 2, 3, 4)


@pytest.mark.parametrize("content", list(CONTENTS))
@pytest.mark.parametrize("shape", SHAPES, ids=[f"{w}x{h}" for w, h in SHAPES])
def test_gray_frame_equals_the_twin(nmi, shape, content):
    w, h = shape
    make, bits = CONTENTS[content]
    layouts = [(extra, off) for extra in (None, 2, 10, 64) for off in (0, 2, 6)]
    with nmi.NmiContext(w, h) as ctx:
        check_frame(ctx, make(w, h), bits, layouts)


@pytest.mark.parametrize("count", PLANTED)
def test_counts_where_a_16_bit_counter_wraps(nmi, count):
    w, h = 256, 257
    px = tnp.planted(w, h, count, value=30000, seed=count)
    assert tnp.histogram(px, 16)[30000] == count
    with nmi.NmiContext(w, h) as ctx:
        check_frame(ctx, px, 16, [(None, 0), (10, 2)])


def test_the_default_tone_map_is_shift_16(nmi):
    w, h = 64, 48
    px = tnp.uniform(w, h, 8)
    d = dev(tnp.pack16(px))
    with nmi.NmiContext(w, h) as ctx:
        assert (ctx.gray_frame(d, capi.FRAME_GRAY16).cpu().numpy() == px >> 8).all()
        tm = capi.ToneMap()
        assert ctx._lib.nmi_tone_map_default(tm) == capi.NMI_OK
        assert (tm.mode, tm.bits, list(tm.reserved), tm.d_lut) == (capi.TONE_SHIFT, 16, [0] * 5, None)
        ctx.set_tone_map(capi.ToneMap.equalize())
        assert (ctx.gray_frame(d, capi.FRAME_GRAY16).cpu().numpy() != px >> 8).any()
        ctx.set_tone_map(None)
        assert (ctx.gray_frame(d, capi.FRAME_GRAY16).cpu().numpy() == px >> 8).all()


def test_a_frame_of_more_than_one_histogram_chunk(nmi):
    """2896 x 1450 = 4,199,200 pixels: more than the 1024 workgroups x 512 runs of 8 pixels the histogram kernel covers at once, so
    its workgroups take a second chunk (nmi_tone.hip)."""
    w, h = 2896, 1450
    assert w * h > 1024 * 512 * 8
    px = tnp.uniform(w, h, 11)
    px[:, : w // 2] = (7000 + px[:, : w // 2] % 400).astype(np.uint16)   # half the frame a narrow band
    d = dev(tnp.pack16(px))
    with nmi.NmiContext(w, h) as ctx:
        for tm in (tnp.tone(tnp.EQUALIZE, 16), tnp.tone(tnp.PERCENTILE, 15, p_lo=100, p_hi=100)):
            ctx.set_tone_map(tnp.capi_tone(capi, tm))
            want_lut, want_pair = tnp.table(tm, tnp.histogram(px, tm["bits"]))
            lut, pair = ctx.tone_lut(d)
            assert pair == want_pair and (lut.cpu().numpy() == want_lut).all()
            assert (ctx.gray_frame(d, capi.FRAME_GRAY16).cpu().numpy() == want_lut[px]).all()
