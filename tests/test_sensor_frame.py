"""GPU tests (-m gpu) of nmi_gray_frame on the raw sensor formats (include/nmi_hip.h): packed YUV 4:2:2 and the four Bayer
patterns, from 2x2 up, dense and pitched rows, source bases 0, 1 and 3 bytes into their allocation -- == the numpy twin
(tests/helpers/sensor_np.py); rejected arguments leave the output untouched."""
import numpy as np
import pytest

from helpers import sensor_np as snp
from orbslam2_nmi_amd import capi

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

# 2x2, 3x2, 2x3: every pixel reflects; 5x3: one interior pixel, a ragged quad; 8x4: two whole quads; 64x48: interior quads on the
# vector path; 1241x376: more than one block per row, an odd width
SHAPES = [(2, 2), (3, 2), (2, 3), (5, 3), (8, 4), (64, 48), (1241, 376)]


@pytest.fixture(scope="module")
def nmi():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    import orbslam2_nmi_amd as m
    m.load_library()
    return m


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def test_the_ids_are_the_headers():
    assert (capi.FRAME_YUYV, capi.FRAME_UYVY) == (snp.YUYV, snp.UYVY) == (16, 17)
    assert (capi.FRAME_BAYER_RGGB, capi.FRAME_BAYER_GRBG, capi.FRAME_BAYER_GBRG, capi.FRAME_BAYER_BGGR) == (32, 33, 34, 35)
    assert {f: capi.FRAME_BYTES_PER_PIXEL[f] for f in snp.BPP} == snp.BPP


@pytest.mark.parametrize("fmt", list(snp.FORMATS.values()), ids=list(snp.FORMATS))
@pytest.mark.parametrize("shape", SHAPES, ids=[f"{w}x{h}" for w, h in SHAPES])
def test_gray_frame_equals_the_twin(nmi, shape, fmt):
    w, h = shape
    rng = np.random.default_rng(fmt * 7 + w)
    img = rng.integers(0, 256, (h, w), dtype=np.uint8)
    dense = w * snp.BPP[fmt]
    with nmi.NmiContext(w, h) as ctx:
        for extra in (None, 1, 5, 64):               # dense (pitch 0), then pitch = W * bpp + extra
            pitch = 0 if extra is None else dense + extra
            for off in (0, 1, 3):
                buf = snp.pack(img, fmt, pitch, off, seed=off)
                d = dev(buf)
                out = torch.full((h, w), 0xAB, dtype=torch.uint8, device="cuda")
                ctx.gray_frame(d[off:], fmt, pitch, out=out)
                want = snp.to_gray(buf, fmt, w, h, pitch, off)
                got = out.cpu().numpy()
                assert (got == want).all(), (fmt, pitch, off, np.argwhere(got != want)[:5])


@pytest.mark.parametrize("shape", [(64, 48), (5, 3)], ids=["64x48", "5x3"])
def test_pattern_and_luma_byte_matter(nmi, shape):
    w, h = shape
    rgb = snp.chroma_frame(w, h, seed=2)
    with nmi.NmiContext(w, h) as ctx:
        buf = snp.pack(snp.mosaic(rgb, snp.RGGB), snp.RGGB)
        grays = [ctx.gray_frame(dev(buf), f).cpu().numpy() for f in snp.BAYER_FORMATS.values()]
        for i, f in enumerate(snp.BAYER_FORMATS.values()):
            assert (grays[i] == snp.to_gray(buf, f, w, h)).all()
            for j in range(i):
                assert (grays[i] != grays[j]).any()
        yuv = snp.pack(rgb[..., 1].copy(), snp.YUYV, seed=4)
        a, b = ctx.gray_frame(dev(yuv), snp.YUYV).cpu().numpy(), ctx.gray_frame(dev(yuv), snp.UYVY).cpu().numpy()
        assert (a == rgb[..., 1]).all() and (b == snp.to_gray(yuv, snp.UYVY, w, h)).all() and (a != b).any()


def test_flat_and_saturated_mosaics(nmi):
    w, h = 20, 6
    with nmi.NmiContext(w, h) as ctx:
        for g in (0, 1, 128, 255):
            buf = dev(np.full(h * w, g, np.uint8))
            for f in snp.BAYER_FORMATS.values():
                assert (ctx.gray_frame(buf, f).cpu().numpy() == g).all()


def test_invalid_arguments_are_rejected_and_leave_the_output(nmi):
    w, h = 64, 48
    E = capi.ERR_INVALID_ARGUMENT
    out = torch.full((h, w), 0xAB, dtype=torch.uint8, device="cuda")
    src = torch.zeros(h * w * 4 + 256, dtype=torch.uint8, device="cuda")
    sp, op = src.data_ptr(), out.data_ptr()
    with nmi.NmiContext(w, h) as ctx:
        lib = ctx._lib
        for fmt in (*range(5, 16), *range(18, 32), 36):
            assert lib.nmi_gray_frame(ctx._h, sp, fmt, 0, op) == E, fmt
        for fmt in snp.YUV_FORMATS.values():         # pitch < 2 W
            for pitch in (1, w, 2 * w - 1, -2 * w):
                assert lib.nmi_gray_frame(ctx._h, sp, fmt, pitch, op) == E, (fmt, pitch)
        for fmt in snp.BAYER_FORMATS.values():
            for pitch in (1, w - 1, -w):
                assert lib.nmi_gray_frame(ctx._h, sp, fmt, pitch, op) == E, (fmt, pitch)
        # d_gray overlapping the source span: its first byte, its last byte, inside a pitched frame's padding
        assert lib.nmi_gray_frame(ctx._h, sp, snp.YUYV, 0, sp) == E
        assert lib.nmi_gray_frame(ctx._h, sp, snp.YUYV, 0, sp + h * w * 2 - 1) == E
        assert lib.nmi_gray_frame(ctx._h, sp, snp.UYVY, 2 * w + 16, sp + 2 * w + 1) == E
        assert lib.nmi_gray_frame(ctx._h, sp, snp.RGGB, 0, sp + h * w - 1) == E
        assert lib.nmi_gray_frame(ctx._h, sp + 100, snp.BGGR, 0, sp + 100 - h * w + 1) == E
        assert lib.nmi_gray_frame(ctx._h, sp, snp.GRBG, w + 16, sp + w + 1) == E
        with pytest.raises(capi.NmiError):
            ctx.gray_frame(src, 18)
        # just outside: accepted (the grey frame ends where the source begins)
        g = torch.zeros(h * w + h * w * 2, dtype=torch.uint8, device="cuda")
        assert lib.nmi_gray_frame(ctx._h, g.data_ptr() + h * w, snp.YUYV, 0, g.data_ptr()) == capi.NMI_OK
        ctx.synchronize()
    # a mosaic needs two columns and two rows; YUV and grey do not
    other = torch.empty(64, dtype=torch.uint8, device="cuda")
    for cw, ch in ((1, 48), (64, 1), (1, 1)):
        with nmi.NmiContext(cw, ch) as ctx:
            for fmt in snp.BAYER_FORMATS.values():
                assert ctx._lib.nmi_gray_frame(ctx._h, sp, fmt, 0, op) == E, (cw, ch, fmt)
                assert ctx._lib.nmi_gray_frame(ctx._h, sp, fmt, 64, op) == E, (cw, ch, fmt)
            assert ctx._lib.nmi_gray_frame(ctx._h, sp, snp.YUYV, 0, other.data_ptr()) == capi.NMI_OK
            ctx.synchronize()
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 0xAB).all()
