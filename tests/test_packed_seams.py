"""GPU tests (-m gpu) of nmi_unpack_frame past one block column, on every tail run and on every store path (nmi_unpack.hip;
include/nmi_hip.h "Deep frames"), == the model of tests/helpers/packed_np.py on bytes.  A block column of the unpack kernels is
64 lanes x 8 pixels = 512 source pixels:
  * widths from below one run to three block columns, every tail n the layout allows (GRAY16_BE: 1 .. 7; the 12-bit layouts 2,
    4, 6 -- partial runs of 3, 6 and 9 source bytes; the 10-bit ones 4), heights 1 and 5, dense and odd pitches, source bases
    0 .. 3 bytes off a 16-byte boundary, and a factor-3 source across column 512;
  * the container written into a caller's buffer 0, 2, 8 and 10 bytes past a 16-byte boundary at widths 520, 516 and 518: the
    16-byte, the 8-byte and the pixel-by-pixel stores chosen by the base, the bytes around the container untouched;
  * the 16-bit mosaics at 513 .. 1031 sites a row: windows read as they lie on both sides of site 512, reflected first and last
    rows and columns, odd tails;
  * one chain per format at 520 x 8: nmi_gray_frame / nmi_reduce_frame of the source == the same call on the model's container.
tests/test_intake_geometry.py proves on the CPU that the sizes reach those branches."""
import numpy as np
import pytest

from helpers import packed_np as pnp
from helpers import seam_cases as cases
from test_packed_frame import dev_at, layouts, same_under_every_tone_map, unpacked

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

GUARD = 64   # bytes of 0xAB kept on both sides of a caller's container


@pytest.fixture(scope="module")
def nmi():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    import orbslam2_nmi_amd as m
    m.load_library()
    return m


def container_at(ws, hs, off):
    """(whole, out): a 0xAB-filled uint8 device tensor and the int16 [hs, ws] view of it whose first byte lies `off` bytes past a
    16-byte boundary, GUARD or more bytes from both ends."""
    n = 2 * ws * hs
    whole = torch.full((n + 2 * GUARD + 32,), 0xAB, dtype=torch.uint8, device="cuda")
    start = (-whole.data_ptr()) % 16 + GUARD + off
    out = whole[start:start + n].view(torch.int16).view(hs, ws)
    assert out.data_ptr() % 16 == off and out.is_contiguous()
    return whole, out, start


def unpacked_into(ctx, d, fmt, f, pitch, ws, hs, off):
    """nmi_unpack_frame into a caller's container at base offset `off`; the bytes around it must stay 0xAB."""
    whole, out, start = container_at(ws, hs, off)
    assert ctx.unpack_frame(d, fmt, f, pitch, out=out) is out
    got = whole.cpu().numpy()
    n = 2 * ws * hs
    assert (got[:start] == 0xAB).all() and (got[start + n:] == 0xAB).all(), ("written outside the container", fmt, ws, hs, off)
    return got[start:start + n].view("<u2").reshape(hs, ws)


@pytest.mark.parametrize("fmt,width", [(f, w) for f in pnp.LAYOUTS for w in cases.UNPACK_WIDTHS[f]])
def test_unpack_at_every_tail_and_across_block_columns(nmi, fmt, width):
    for h in cases.UNPACK_HEIGHTS:
        with nmi.NmiContext(width, h) as ctx:
            for name, px in pnp.contents(fmt, width, h, seed=h).items():
                for pitch, off in layouts(fmt, width):
                    d = dev_at(pnp.frame(px, fmt, pitch, 0, seed=off), off)
                    got = unpacked(ctx, d, fmt, 1, pitch)
                    assert got.shape == (h, width) and (got == px).all(), (name, h, pitch, off, np.argwhere(got != px)[:5])


@pytest.mark.parametrize("fmt", pnp.LAYOUTS)
def test_unpack_a_factor_3_source_across_the_seam(nmi, fmt):
    w, h = cases.UNPACK_FACTOR3
    ws, hs = 3 * w, 3 * h
    with nmi.NmiContext(w, h) as ctx:
        for name, px in pnp.contents(fmt, ws, hs, seed=3).items():
            for pitch, off in layouts(fmt, ws):
                d = dev_at(pnp.frame(px, fmt, pitch, 0, seed=off), off)
                got = unpacked(ctx, d, fmt, 3, pitch)
                assert got.shape == (hs, ws) and (got == px).all(), (name, pitch, off, np.argwhere(got != px)[:5])


@pytest.mark.parametrize("fmt,width", [(f, w) for f in pnp.LAYOUTS for w in cases.out_widths(f)])
def test_the_store_path_follows_the_containers_base(nmi, fmt, width):
    h = cases.OUT_HEIGHT
    with nmi.NmiContext(width, h) as ctx:
        for name, px in pnp.contents(fmt, width, h, seed=width).items():
            pitch, off = layouts(fmt, width)[-1]
            d = dev_at(pnp.frame(px, fmt, pitch, 0, seed=1), off)
            for base in cases.OUT_BASES:
                got = unpacked_into(ctx, d, fmt, 1, pitch, width, h, base)
                assert (got == px).all(), (name, base, np.argwhere(got != px)[:5])


@pytest.mark.parametrize("size", cases.BAYER_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("pattern", list(pnp.BAYER16))
def test_bayer16_across_block_columns(nmi, pattern, size):
    w, h = size
    fmt = pnp.BAYER16[pattern]
    sites = {"random": pnp.random_pixels(fmt, w, h, seed=w), "ones": np.full((h, w), 65535, np.uint16)}
    with nmi.NmiContext(w, h) as ctx:
        for name, m in sites.items():
            want = pnp.bayer16_gray(m, fmt)
            if name == "ones":
                assert (want == 65535).all()
            for pitch, off in layouts(fmt, w):
                d = dev_at(pnp.frame(m, fmt, pitch, 0, seed=off), off)
                got = unpacked(ctx, d, fmt, 1, pitch)
                assert (got == want).all(), (name, pitch, off, np.argwhere(got != want)[:5])
            if size == cases.BAYER_OUT_SIZE:
                pitch, off = layouts(fmt, w)[-1]
                d = dev_at(pnp.frame(m, fmt, pitch, 0, seed=2), off)
                for base in cases.OUT_BASES:
                    got = unpacked_into(ctx, d, fmt, 1, pitch, w, h, base)
                    assert (got == want).all(), (name, base, np.argwhere(got != want)[:5])


@pytest.mark.parametrize("fmt", pnp.FORMATS)
def test_a_chain_at_a_seam_width(nmi, fmt):
    """Every tone map (SHIFT and EQUALIZE among them) on the source == on GRAY16 given the model's container."""
    w, h = cases.CHAIN_SIZE
    px = pnp.random_pixels(fmt, w, h, seed=fmt)
    pitch, off = layouts(fmt, w)[-1]
    buf = pnp.frame(px, fmt, pitch, 0, seed=4)
    with nmi.NmiContext(w, h) as ctx:
        seen = same_under_every_tone_map(ctx, dev_at(buf, off), fmt, 1, pitch, pnp.container(buf, fmt, w, h, pitch), pnp.BITS[fmt])
    assert {"shift", "equalize"} <= set(seen) and (seen["shift"] != seen["equalize"]).any()
