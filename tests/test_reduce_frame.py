"""GPU tests (-m gpu) of nmi_reduce_frame (include/nmi_hip.h): every format and factor, dense and pitched rows, source bases 0, 1
and 3 bytes into their allocation, output widths that are and are not multiples of a lane's run, the camera sizes the reference
names -- == the numpy twin (tests/helpers/reduce_np.py); every possible block sum; factor 1 == nmi_gray_frame; the fused colour
reduction == nmi_gray_frame at full size followed by the grey reduction; masks; rejected arguments leave the outputs untouched."""
import numpy as np
import pytest

from helpers import color_np as cnp
from helpers import reduce_np as rnp
from orbslam2_nmi_amd import capi

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

FMT_IDS = list(cnp.FORMATS)
FMTS = list(cnp.FORMATS.values())


@pytest.fixture(scope="module")
def nmi():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    import orbslam2_nmi_amd as m
    m.load_library()
    return m


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def image(rng, fmt, w, h):
    return rng.integers(0, 256, (h, w) if fmt == cnp.GRAY else (h, w, 3), dtype=np.uint8)


def run(ctx, buf, off, fmt, f, pitch):
    w, h = ctx.width, ctx.height
    out = torch.full((h, w), 0xAB, dtype=torch.uint8, device="cuda")
    ctx.reduce_frame(dev(buf)[off:], fmt, f, pitch, out=out)
    return out.cpu().numpy()


@pytest.mark.parametrize("fmt", FMTS, ids=FMT_IDS)
@pytest.mark.parametrize("f", [1, 2, 3, 4])
@pytest.mark.parametrize("shape", [(208, 36), (203, 37)], ids=["208x36", "203x37"])
def test_reduce_frame_equals_the_twin(nmi, shape, f, fmt):
    """Output 208 wide: a multiple of every run (4, 8, 16); 203: a ragged last run, byte stores."""
    w, h = shape
    rng = np.random.default_rng(fmt * 7 + w + f)
    img = image(rng, fmt, f * w, f * h)
    dense = f * w * cnp.BPP[fmt]
    with nmi.NmiContext(w, h) as ctx:
        for extra in (None, 1, 5, 64):               # dense (pitch 0), then pitch = f * W * bpp + extra
            pitch = 0 if extra is None else dense + extra
            for off in (0, 1, 3):
                buf = cnp.pack(img, fmt, pitch, off, seed=off)
                got = run(ctx, buf, off, fmt, f, pitch)
                want = rnp.reduce_frame(buf, fmt, w, h, f, pitch, off)
                assert (got == want).all(), (fmt, f, pitch, off, np.argwhere(got != want)[:5])
        if fmt != cnp.GRAY:                          # the order matters: RGB != BGR on a frame with chroma
            swapped = {cnp.RGB: cnp.BGR, cnp.BGR: cnp.RGB, cnp.RGBA: cnp.BGRA, cnp.BGRA: cnp.RGBA}[fmt]
            buf = cnp.pack(img, fmt)
            other = run(ctx, buf, 0, swapped, f, 0)
            assert (other == rnp.reduce_frame(buf, swapped, w, h, f)).all()
            assert (other != rnp.reduce_frame(buf, fmt, w, h, f)).any()


# (source width, source height, factor, output width, output height): the reference's camera sizes
CAMERAS = [(1920, 1080, 2, 960, 540), (3840, 2160, 4, 960, 540), (2544, 1440, 3, 848, 480), (1241, 376, 2, 620, 188), (1242, 375, 3, 414, 125)]


@pytest.mark.parametrize("fmt", FMTS, ids=FMT_IDS)
@pytest.mark.parametrize("cam", CAMERAS, ids=[f"{c[0]}x{c[1]}-to-{c[3]}x{c[4]}" for c in CAMERAS])
def test_camera_sizes(nmi, cam, fmt):
    """The source is as wide as the camera makes it; where that is more than f * W pixels (1241 at f = 2) its real pitch crops it."""
    sw, sh, f, w, h = cam
    assert w == sw // f and h == sh // f
    rng = np.random.default_rng(sw + fmt)
    img = image(rng, fmt, sw, sh)
    real = sw * cnp.BPP[fmt]                          # the camera's dense rows
    cropped = sw != f * w
    with nmi.NmiContext(w, h) as ctx:
        for pitch in ((real,) if cropped else (0, real + 64)):
            buf = cnp.pack(img, fmt, pitch)
            got = run(ctx, buf, 0, fmt, f, pitch)
            want = rnp.reduce_frame(buf, fmt, w, h, f, pitch)
            assert got.shape == (h, w)
            assert (got == want).all(), (cam, fmt, pitch, np.argwhere(got != want)[:5])
            if cropped:                               # the same as reducing the frame without its spare column
                grey = cnp.to_gray(buf, fmt, sw, sh)
                assert (got == rnp.reduce_gray(grey[:f * h, :f * w], f)).all()


@pytest.mark.parametrize("fmt", [cnp.GRAY, cnp.RGB, cnp.BGRA], ids=["gray", "rgb", "bgra"])
@pytest.mark.parametrize("f", [2, 3, 4])
def test_every_block_sum(nmi, f, fmt):
    """A frame in whose blocks every sum 0 .. 255 f^2 occurs (colour: R = G = B, which the grey rule maps to itself)."""
    w, h = 96, 48
    g = rnp.every_sum_frame(f, w, h, seed=f)
    sums = rnp.block_sums(g, f)
    assert len(np.unique(sums)) == 255 * f * f + 1
    img = g if fmt == cnp.GRAY else np.stack([g, g, g], -1)
    with nmi.NmiContext(w, h) as ctx:
        for pitch, off in ((0, 0), (f * w * cnp.BPP[fmt] + 3, 1)):   # the 16-byte loads, and the byte loads
            buf = cnp.pack(img, fmt, pitch, off)
            got = run(ctx, buf, off, fmt, f, pitch)
            assert (got == rnp.round_sum(sums, f)).all()
            assert (got == rnp.reduce_frame(buf, fmt, w, h, f, pitch, off)).all()


@pytest.mark.parametrize("fmt", FMTS, ids=FMT_IDS)
def test_factor_one_is_gray_frame(nmi, fmt):
    w, h = 322, 120
    img = image(np.random.default_rng(fmt), fmt, w, h)
    with nmi.NmiContext(w, h) as ctx:
        for pitch, off in ((0, 0), (w * cnp.BPP[fmt] + 5, 3)):
            buf = cnp.pack(img, fmt, pitch, off)
            d = dev(buf)
            a = ctx.reduce_frame(d[off:], fmt, 1, pitch).cpu().numpy()
            b = ctx.gray_frame(d[off:], fmt, pitch).cpu().numpy()
            assert (a == b).all() and (a == cnp.to_gray(buf, fmt, w, h, pitch, off)).all()


@pytest.mark.parametrize("fmt", cnp.COLOR_FORMATS, ids=["bgr", "rgb", "bgra", "rgba"])
@pytest.mark.parametrize("f", [2, 3, 4])
def test_fused_colour_reduction_is_gray_frame_then_the_grey_reduction(nmi, f, fmt):
    w, h = 424, 120
    img = image(np.random.default_rng(fmt * 3 + f), fmt, f * w, f * h)
    pitch = f * w * cnp.BPP[fmt] + 16
    buf = dev(cnp.pack(img, fmt, pitch))
    with nmi.NmiContext(w, h) as ctx, nmi.NmiContext(f * w, f * h) as full:
        fused = ctx.reduce_frame(buf, fmt, f, pitch)
        grey = full.gray_frame(buf, fmt, pitch)                      # [f*H, f*W] dense grey
        chained = ctx.reduce_frame(grey.reshape(-1), cnp.GRAY, f)
        assert (fused.cpu().numpy() == chained.cpu().numpy()).all()


@pytest.mark.parametrize("f", [1, 2, 3, 4])
@pytest.mark.parametrize("shape", [(208, 36), (203, 37)], ids=["208x36", "203x37"])
def test_mask_equals_the_twin(nmi, shape, f):
    w, h = shape
    rng = np.random.default_rng(f + w)
    img = image(rng, cnp.RGB, f * w, f * h)
    m = (rng.random((f * h, f * w)) < 0.93).astype(np.uint8) * rng.integers(1, 256, (f * h, f * w), dtype=np.uint8)
    m[: f * 3] = 1                                                   # some rows wholly set
    m[f * 5: f * 7, f * 10: f * 40] = 0                              # a hole
    buf = cnp.pack(img, cnp.RGB)
    with nmi.NmiContext(w, h) as ctx:
        out_mask = torch.full((h, w), 0xCD, dtype=torch.uint8, device="cuda")
        frame, mask = ctx.reduce_frame(dev(buf), cnp.RGB, f, src_mask=dev(m), out_mask=out_mask)
        assert mask is out_mask
        want = rnp.reduce_mask(m, f)
        assert 0 < want.sum() < want.size
        assert (mask.cpu().numpy() == want).all()
        assert (frame.cpu().numpy() == rnp.reduce_frame(buf, cnp.RGB, w, h, f)).all()
        assert (ctx.reduce_frame(dev(buf), cnp.RGB, f, src_mask=dev(m.astype(bool)))[1].cpu().numpy() == want).all()
        # without the mask pointers: the frame alone, and nothing else is written (the output sits between two guard rows)
        guard = torch.full((h + 2, w), 0xEE, dtype=torch.uint8, device="cuda")
        rc = ctx._lib.nmi_reduce_frame(ctx._h, dev(buf).data_ptr(), cnp.RGB, 0, f, None, guard[1:].data_ptr(), None)
        assert rc == capi.NMI_OK
        ctx.synchronize()
        gnp = guard.cpu().numpy()
        assert (gnp[0] == 0xEE).all() and (gnp[h + 1] == 0xEE).all()
        assert (gnp[1:h + 1] == rnp.reduce_frame(buf, cnp.RGB, w, h, f)).all()


def test_invalid_arguments_are_rejected_and_leave_the_outputs(nmi):
    w, h, f = 64, 48, 2
    with nmi.NmiContext(w, h) as ctx:
        lib = ctx._lib
        fw, fh = f * w, f * h
        src = torch.zeros(fh * fw * 4 + 256, dtype=torch.uint8, device="cuda")
        smask = torch.ones(fh * fw, dtype=torch.uint8, device="cuda")
        out = torch.full((h, w), 0xAB, dtype=torch.uint8, device="cuda")
        omask = torch.full((h, w), 0xCD, dtype=torch.uint8, device="cuda")
        sp, mp, op, omp = src.data_ptr(), smask.data_ptr(), out.data_ptr(), omask.data_ptr()
        E = capi.ERR_INVALID_ARGUMENT
        call = lib.nmi_reduce_frame
        assert call(None, sp, cnp.RGB, 0, f, mp, op, omp) == E
        assert call(ctx._h, None, cnp.RGB, 0, f, mp, op, omp) == E
        assert call(ctx._h, sp, cnp.RGB, 0, f, mp, None, omp) == E
        for fmt in (-1, 5, 99):
            assert call(ctx._h, sp, fmt, 0, f, mp, op, omp) == E, fmt
        for bad in (0, -1, 5, 8):
            assert call(ctx._h, sp, cnp.RGB, 0, bad, mp, op, omp) == E, bad
        for fmt, bpp in cnp.BPP.items():
            for pitch in (1, fw * bpp - 1, w * bpp, -1, -fw * bpp):          # (W * bpp: a pitch of the search size is too small)
                assert call(ctx._h, sp, fmt, pitch, f, mp, op, omp) == E, (fmt, pitch)
        assert call(ctx._h, sp, cnp.RGB, 0, f, mp, op, None) == E             # exactly one of the two mask pointers
        assert call(ctx._h, sp, cnp.RGB, 0, f, None, op, omp) == E
        # overlaps: an output on the source's first byte, on its last byte, inside a pitched source's padding; on the source mask; on
        # the other output
        last = (fh - 1) * fw * 3 + fw * 3 - 1
        assert call(ctx._h, sp, cnp.RGB, 0, f, None, sp, None) == E
        assert call(ctx._h, sp, cnp.RGB, 0, f, None, sp + last, None) == E
        assert call(ctx._h, sp + h * w, cnp.GRAY, 0, f, None, sp + 1, None) == E
        assert call(ctx._h, sp, cnp.GRAY, fw + 16, f, None, sp + fw + 1, None) == E
        assert call(ctx._h, sp, cnp.RGB, 0, f, mp, op, sp + 5) == E
        assert call(ctx._h, sp, cnp.RGB, 0, f, mp, mp, omp) == E
        assert call(ctx._h, sp, cnp.RGB, 0, f, mp, op, mp + fh * fw - 1) == E
        assert call(ctx._h, sp, cnp.RGB, 0, f, mp, op, op) == E
        assert call(ctx._h, sp, cnp.RGB, 0, f, mp, op, op + h * w - 1) == E
        torch.cuda.synchronize()
        assert (out.cpu().numpy() == 0xAB).all() and (omask.cpu().numpy() == 0xCD).all()
        # just outside: accepted (the grey frame ends where the source begins)
        g = torch.zeros(h * w + fh * fw * 3, dtype=torch.uint8, device="cuda")
        assert call(ctx._h, g.data_ptr() + h * w, cnp.RGB, 0, f, None, g.data_ptr(), None) == capi.NMI_OK
        ctx.synchronize()
        with pytest.raises(capi.NmiError):
            ctx.reduce_frame(src, 7, f)
        with pytest.raises(capi.NmiError):
            ctx.reduce_frame(src, cnp.RGB, 5)
