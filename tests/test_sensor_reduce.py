"""GPU tests (-m gpu) of nmi_reduce_frame on the raw sensor formats (include/nmi_hip.h): packed YUV 4:2:2 and the four Bayer
patterns at factors 2, 3 and 4 -- == the numpy twin (tests/helpers/sensor_np.py: the grey rule on the full-size frame, then
tests/helpers/reduce_np.py's box rule); pitched, offset and cropped sources; the mask; rejected arguments."""
import numpy as np
import pytest

from helpers import reduce_np as rnp
from helpers import sensor_np as snp
from orbslam2_nmi_amd import capi

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

# output sizes.  1x1: one block, every source pixel at an edge; 7x5: ragged quads, all windows at an edge or next to one; 16x12:
# whole quads, interior windows; 310x94: more than one block per row, a ragged last quad, the source one pixel wider than f * W
# (1241 at f = 4) and cropped by its pitch
SHAPES = [(1, 1), (7, 5), (16, 12), (310, 94)]


@pytest.fixture(scope="module")
def nmi():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    import orbslam2_nmi_amd as m
    m.load_library()
    return m


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run(ctx, buf, off, fmt, f, pitch):
    out = torch.full((ctx.height, ctx.width), 0xAB, dtype=torch.uint8, device="cuda")
    ctx.reduce_frame(dev(buf)[off:], fmt, f, pitch, out=out)
    return out.cpu().numpy()


@pytest.mark.parametrize("fmt", list(snp.FORMATS.values()), ids=list(snp.FORMATS))
@pytest.mark.parametrize("f", [2, 3, 4])
@pytest.mark.parametrize("shape", SHAPES, ids=[f"{w}x{h}" for w, h in SHAPES])
def test_reduce_frame_equals_the_twin(nmi, shape, f, fmt):
    w, h = shape
    rng = np.random.default_rng(fmt * 7 + w + f)
    bpp = snp.BPP[fmt]
    spare = 1 if w == 310 else 0                      # source pixels per row beyond f * W
    img = rng.integers(0, 256, (f * h, f * w + spare), dtype=np.uint8)
    real = (f * w + spare) * bpp
    with nmi.NmiContext(w, h) as ctx:
        for pitch in ((real, real + 3) if spare else (0, real + 1, real + 5, real + 64)):
            for off in (0, 1, 3):
                buf = snp.pack(img, fmt, pitch, off, seed=off)
                got = run(ctx, buf, off, fmt, f, pitch)
                want = snp.reduce_frame(buf, fmt, w, h, f, pitch, off)
                assert (got == want).all(), (fmt, f, pitch, off, np.argwhere(got != want)[:5])
                if spare:                             # the same as reducing the frame without its spare column
                    cut = snp.pack(img[:, :f * w].copy(), fmt)
                    assert (got == snp.reduce_frame(cut, fmt, w, h, f)).all()


@pytest.mark.parametrize("f", [2, 3, 4])
def test_fused_reduction_is_gray_frame_then_the_grey_reduction(nmi, f):
    w, h = 44, 9
    rgb = snp.chroma_frame(f * w, f * h, seed=f)
    with nmi.NmiContext(w, h) as ctx, nmi.NmiContext(f * w, f * h) as full:
        for fmt in (snp.GRBG, snp.BGGR, snp.UYVY):
            img = snp.mosaic(rgb, fmt) if snp.is_bayer(fmt) else rgb[..., 0].copy()
            pitch = f * w * snp.BPP[fmt] + 16
            buf = dev(snp.pack(img, fmt, pitch))
            fused = ctx.reduce_frame(buf, fmt, f, pitch)
            grey = full.gray_frame(buf, fmt, pitch)
            chained = ctx.reduce_frame(grey.reshape(-1), capi.FRAME_GRAY, f)
            assert (fused.cpu().numpy() == chained.cpu().numpy()).all()


def test_factor_one_is_gray_frame(nmi):
    w, h = 23, 10
    img = np.random.default_rng(1).integers(0, 256, (h, w), dtype=np.uint8)
    with nmi.NmiContext(w, h) as ctx:
        for fmt in snp.FORMATS.values():
            buf = snp.pack(img, fmt, w * snp.BPP[fmt] + 5, 3)
            got = ctx.reduce_frame(dev(buf)[3:], fmt, 1, w * snp.BPP[fmt] + 5).cpu().numpy()
            assert (got == snp.to_gray(buf, fmt, w, h, w * snp.BPP[fmt] + 5, 3)).all()


def test_the_source_mask_is_reduced_as_before(nmi):
    w, h, f = 29, 7, 3
    rng = np.random.default_rng(8)
    img = rng.integers(0, 256, (f * h, f * w), dtype=np.uint8)
    m = (rng.random((f * h, f * w)) < 0.95).astype(np.uint8) * rng.integers(1, 256, (f * h, f * w), dtype=np.uint8)
    buf = snp.pack(img, snp.GBRG)
    with nmi.NmiContext(w, h) as ctx:
        frame, mask = ctx.reduce_frame(dev(buf), snp.GBRG, f, src_mask=dev(m))
        want = rnp.reduce_mask(m, f)
        assert 0 < want.sum() < want.size
        assert (mask.cpu().numpy() == want).all()
        assert (frame.cpu().numpy() == snp.reduce_frame(buf, snp.GBRG, w, h, f)).all()


def test_invalid_arguments_are_rejected_and_leave_the_outputs(nmi):
    w, h, f = 64, 48, 2
    with nmi.NmiContext(w, h) as ctx:
        fw, fh = f * w, f * h
        src = torch.zeros(fh * fw * 2 + 256, dtype=torch.uint8, device="cuda")
        out = torch.full((h, w), 0xAB, dtype=torch.uint8, device="cuda")
        sp, op = src.data_ptr(), out.data_ptr()
        E = capi.ERR_INVALID_ARGUMENT
        call = ctx._lib.nmi_reduce_frame
        for fmt in (*range(5, 16), *range(18, 32), 36):
            assert call(ctx._h, sp, fmt, 0, f, None, op, None) == E, fmt
        for fmt, bpp in snp.BPP.items():
            for pitch in (1, fw * bpp - 1, w * bpp, -1):
                assert call(ctx._h, sp, fmt, pitch, f, None, op, None) == E, (fmt, pitch)
            for bad in (0, 5):
                assert call(ctx._h, sp, fmt, 0, bad, None, op, None) == E, (fmt, bad)
        assert call(ctx._h, sp, snp.YUYV, 0, f, None, sp + fh * fw * 2 - 1, None) == E
        assert call(ctx._h, sp, snp.RGGB, 0, f, None, sp + fh * fw - 1, None) == E
        assert call(ctx._h, sp, snp.RGGB, fw + 16, f, None, sp + fw + 1, None) == E
        torch.cuda.synchronize()
        assert (out.cpu().numpy() == 0xAB).all()
        g = torch.zeros(h * w + fh * fw, dtype=torch.uint8, device="cuda")
        assert call(ctx._h, g.data_ptr() + h * w, snp.BGGR, 0, f, None, g.data_ptr(), None) == capi.NMI_OK
        ctx.synchronize()
