"""GPU tests (-m gpu) of nmi_gray_frame (include/nmi_hip.h): every format, dense and pitched rows, source bases 0, 1 and 3 bytes
into their allocation, widths that are and are not multiples of 4 -- == the numpy twin (tests/helpers/color_np.py); all 2^24
(R, G, B) triples; rejected arguments leave the output untouched."""
import numpy as np
import pytest

from helpers import color_np as cnp
from orbslam2_nmi_amd import capi

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SHAPES = [(640, 480), (1241, 376), (64, 48)]


@pytest.fixture(scope="module")
def nmi():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    import orbslam2_nmi_amd as m
    m.load_library()
    return m


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("fmt", list(cnp.FORMATS.values()), ids=list(cnp.FORMATS))
@pytest.mark.parametrize("shape", SHAPES, ids=[f"{w}x{h}" for w, h in SHAPES])
def test_gray_frame_equals_the_twin(nmi, shape, fmt):
    w, h = shape
    rng = np.random.default_rng(fmt * 7 + w)
    img = rng.integers(0, 256, (h, w) if fmt == cnp.GRAY else (h, w, 3), dtype=np.uint8)
    dense = w * cnp.BPP[fmt]
    with nmi.NmiContext(w, h) as ctx:
        for extra in (None, 1, 5, 64):               # dense (pitch 0), then pitch = W * bpp + extra
            pitch = 0 if extra is None else dense + extra
            for off in (0, 1, 3):
                buf = cnp.pack(img, fmt, pitch, off, seed=off)
                d = dev(buf)
                out = torch.full((h, w), 0xAB, dtype=torch.uint8, device="cuda")
                ctx.gray_frame(d[off:], fmt, pitch, out=out)
                want = cnp.to_gray(buf, fmt, w, h, pitch, off)
                got = out.cpu().numpy()
                assert (got == want).all(), (fmt, pitch, off, np.argwhere(got != want)[:5])
        if fmt != cnp.GRAY:                          # the order matters: RGB != BGR on a frame with chroma
            swapped = {cnp.RGB: cnp.BGR, cnp.BGR: cnp.RGB, cnp.RGBA: cnp.BGRA, cnp.BGRA: cnp.RGBA}[fmt]
            buf = cnp.pack(img, fmt)
            other = ctx.gray_frame(dev(buf), swapped).cpu().numpy()
            assert (other == cnp.to_gray(buf, swapped, w, h)).all()
            assert (other != cnp.to_gray(buf, fmt, w, h)).any()


@pytest.mark.parametrize("fmt", cnp.COLOR_FORMATS, ids=["bgr", "rgb", "bgra", "rgba"])
def test_every_rgb_triple(nmi, fmt):
    w, h = 2048, 512                                 # 2^20 pixels: 16 frames hold the 2^24 triples
    n = w * h
    with nmi.NmiContext(w, h) as ctx:
        out = torch.empty((h, w), dtype=torch.uint8, device="cuda")
        for k in range((1 << 24) // n):
            t = cnp.all_triples(k * n, n)
            buf = cnp.pack(t.reshape(h, w, 3), fmt, seed=k)
            ctx.gray_frame(dev(buf), fmt, out=out)
            want = cnp.gray_of(t[:, 0], t[:, 1], t[:, 2]).reshape(h, w)
            assert (out.cpu().numpy() == want).all(), k


def test_invalid_arguments_are_rejected_and_leave_the_output(nmi):
    w, h = 64, 48
    with nmi.NmiContext(w, h) as ctx:
        lib = ctx._lib
        src = torch.zeros(h * w * 4 + 256, dtype=torch.uint8, device="cuda")
        out = torch.full((h, w), 0xAB, dtype=torch.uint8, device="cuda")
        sp, op = src.data_ptr(), out.data_ptr()
        E = capi.ERR_INVALID_ARGUMENT
        assert lib.nmi_gray_frame(None, sp, cnp.RGB, 0, op) == E
        assert lib.nmi_gray_frame(ctx._h, None, cnp.RGB, 0, op) == E
        assert lib.nmi_gray_frame(ctx._h, sp, cnp.RGB, 0, None) == E
        for fmt in (-1, 5, 99):
            assert lib.nmi_gray_frame(ctx._h, sp, fmt, 0, op) == E, fmt
        for fmt, bpp in cnp.BPP.items():
            for pitch in (1, w * bpp - 1, -1, -w * bpp):
                assert lib.nmi_gray_frame(ctx._h, sp, fmt, pitch, op) == E, (fmt, pitch)
        # d_gray overlapping the source rows: the source's first byte, its last byte, inside a pitched frame's padding
        assert lib.nmi_gray_frame(ctx._h, sp, cnp.RGB, 0, sp) == E
        assert lib.nmi_gray_frame(ctx._h, sp, cnp.RGB, 0, sp + h * w * 3 - 1) == E
        assert lib.nmi_gray_frame(ctx._h, sp + 100, cnp.GRAY, 0, sp + 100 - h * w + 1) == E
        assert lib.nmi_gray_frame(ctx._h, sp, cnp.GRAY, w + 16, sp + w + 1) == E
        torch.cuda.synchronize()
        assert (out.cpu().numpy() == 0xAB).all()
        # just outside: accepted (the grey frame ends where the source begins)
        g = torch.zeros(h * w + h * w * 3, dtype=torch.uint8, device="cuda")
        assert lib.nmi_gray_frame(ctx._h, g.data_ptr() + h * w, cnp.RGB, 0, g.data_ptr()) == capi.NMI_OK
        ctx.synchronize()
        with pytest.raises(capi.NmiError):
            ctx.gray_frame(src, 7)
