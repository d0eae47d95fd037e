"""GPU tests (-m gpu: they need a context, and fault nothing) of what the deep raw formats refuse (include/nmi_hip.h "Deep
frames"): every rejection is NMI_ERR_INVALID_ARGUMENT before anything is enqueued, with the outputs untouched; odd packed
pitches and bases are accepted; nmi_unpack_frame takes the nine formats only; the ids other tests hold unknown stay unknown."""
import numpy as np
import pytest

from helpers import packed_np as pnp
from orbslam2_nmi_amd import capi

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

W, H = 24, 6
E, OK = capi.ERR_INVALID_ARGUMENT, capi.NMI_OK
UNKNOWN = [-1, *range(5, 16), *range(18, 32), 36, 47, 49, 51, 60, 99]
EIGHT_BIT = [capi.FRAME_GRAY, capi.FRAME_BGR, capi.FRAME_RGBA, capi.FRAME_YUYV, capi.FRAME_BAYER_GRBG]


@pytest.fixture(scope="module")
def nmi():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    import orbslam2_nmi_amd as m
    m.load_library()
    return m


class Outputs:
    """A grey frame, a mask and a container, filled with a pattern no refused call may disturb."""

    def __init__(self, w, h, f=4):
        self.gray = torch.full((h, w), 0xAB, dtype=torch.uint8, device="cuda")
        self.mask = torch.full((h, w), 0xAB, dtype=torch.uint8, device="cuda")
        self.cont = torch.full((f * h, f * w), 0x5A5A, dtype=torch.int16, device="cuda")

    def untouched(self):
        torch.cuda.synchronize()
        return bool((self.gray == 0xAB).all() and (self.mask == 0xAB).all() and (self.cont == 0x5A5A).all())


def every_entry(ctx, sp, fmt, pitch, f, out, src_mask=None):
    """The return codes of nmi_unpack_frame, nmi_reduce_frame (with and without its mask pair) and, at factor 1, nmi_gray_frame."""
    lib, h = ctx._lib, ctx._h
    rc = [lib.nmi_unpack_frame(h, sp, fmt, pitch, f, out.cont.data_ptr()),
          lib.nmi_reduce_frame(h, sp, fmt, pitch, f, None, out.gray.data_ptr(), None)]
    if src_mask is not None:
        rc.append(lib.nmi_reduce_frame(h, sp, fmt, pitch, f, src_mask.data_ptr(), out.gray.data_ptr(), out.mask.data_ptr()))
    if f == 1:
        rc.append(lib.nmi_gray_frame(h, sp, fmt, pitch, out.gray.data_ptr()))
    return rc


def test_widths_that_are_not_whole_groups(nmi):
    """Contexts of 6 and 7 columns: 10-bit formats need f W % 4 == 0, 12-bit ones f W % 2 == 0."""
    src = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    for w in (6, 7, 9):
        out = Outputs(w, 3)
        with nmi.NmiContext(w, 3) as ctx, nmi.NmiStream(ctx, 2, 2) as st:
            for f in (1, 2, 3, 4):
                for fmt in pnp.PACKED:
                    ok = pnp.row_bytes(fmt, f * w) > 0
                    assert (f * w) % pnp.GROUP[fmt][0] == 0 if ok else True
                    rcs = every_entry(ctx, src.data_ptr(), fmt, 0, f, out)
                    assert rcs == [OK if ok else E] * len(rcs), (w, f, fmt)
                    assert ctx._lib.nmi_stream_set_frame_reduction(st._h, f, fmt, 0) == (OK if ok else E)
                    assert ctx._lib.nmi_frame_row_bytes(fmt, f * w) == pnp.row_bytes(fmt, f * w)
                    ctx.synchronize()
                    if ok:
                        out = Outputs(w, 3)
                    else:
                        assert out.untouched()


def test_pitch_alignment_and_overlap(nmi):
    src = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    src_mask = torch.ones((4 * H, 4 * W), dtype=torch.uint8, device="cuda")
    out = Outputs(W, H)
    sp = src.data_ptr() + 4096                                            # (every address below stays inside src)
    with nmi.NmiContext(W, H) as ctx:
        lib, h = ctx._lib, ctx._h
        ctx.set_tone_map(capi.ToneMap.equalize())                         # (a mode with nodes to enqueue)
        for f in (1, 2):
            sm = src_mask[:f * H, :f * W].contiguous()
            for fmt in pnp.FORMATS:
                dense = pnp.row_bytes(fmt, f * W)
                words = pnp.GROUP[fmt][1] == 2
                for pitch in (dense - 1, dense - 2, 1, -dense):           # below the row's bytes
                    assert set(every_entry(ctx, sp, fmt, pitch, f, out, sm)) == {E}, (fmt, pitch)
                if words:                                                 # the 2-byte formats keep GRAY16's rules
                    assert set(every_entry(ctx, sp + 1, fmt, 0, f, out, sm)) == {E}
                    assert set(every_entry(ctx, sp, fmt, dense + 1, f, out, sm)) == {E}
                    assert set(every_entry(ctx, sp + 3, fmt, dense + 3, f, out, sm)) == {E}
                assert set(every_entry(ctx, sp, fmt, 0, 0, out, sm)) == {E} and set(every_entry(ctx, sp, fmt, 0, 5, out, sm)) == {E}
                # an output meeting the source: its first byte, its last, a pitched frame's padding
                span = pnp.span(fmt, f * W, f * H)
                for gp in (sp, sp + span - 1, sp - W * H + 1):
                    assert lib.nmi_reduce_frame(h, sp, fmt, 0, f, None, gp, None) == E, (fmt, gp - sp)
                    assert lib.nmi_reduce_frame(h, sp, fmt, 0, f, sm.data_ptr(), out.gray.data_ptr(), gp) == E
                assert lib.nmi_reduce_frame(h, sp, fmt, dense + 64, f, None, sp + dense + 2, None) == E
                for cp in (sp, sp + span - 1, sp + span - 2, sp - 2 * f * f * W * H + 2):
                    if cp % 2 == 0:
                        assert lib.nmi_unpack_frame(h, sp, fmt, 0, f, cp) == E, (fmt, cp - sp)
                assert lib.nmi_unpack_frame(h, sp, fmt, 0, f, out.cont.data_ptr() + 1) == E      # a container on an odd byte
                assert lib.nmi_unpack_frame(h, None, fmt, 0, f, out.cont.data_ptr()) == E
                assert lib.nmi_unpack_frame(h, sp, fmt, 0, f, None) == E
                assert lib.nmi_unpack_frame(None, sp, fmt, 0, f, out.cont.data_ptr()) == E
                assert lib.nmi_reduce_frame(h, sp, fmt, 0, f, sm.data_ptr(), out.gray.data_ptr(), None) == E   # half a mask pair
        ctx.synchronize()
        assert out.untouched()
        # just outside: accepted (the container begins where the source ends, the grey frame ends where it begins)
        for fmt in (pnp.MONO10P, pnp.RAW12, pnp.GRAY16_BE, pnp.BAYER16["grbg"]):
            span = pnp.span(fmt, W, H)
            assert lib.nmi_unpack_frame(h, sp, fmt, 0, 1, sp + span + span % 2) == OK
            assert lib.nmi_gray_frame(h, sp, fmt, 0, sp - W * H) == OK
        ctx.synchronize()


def test_odd_packed_pitches_and_bases_are_accepted(nmi):
    src = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    out = Outputs(W, H)
    with nmi.NmiContext(W, H) as ctx, nmi.NmiStream(ctx, 2, 2) as st:
        for fmt in pnp.PACKED:
            dense = pnp.row_bytes(fmt, 2 * W)
            for off in (1, 2, 3, 5):
                for pitch in (dense, dense + 1, dense + 3, dense + 7):
                    assert set(every_entry(ctx, src.data_ptr() + off, fmt, pitch, 2, out)) == {OK}, (fmt, off, pitch)
                    assert ctx._lib.nmi_stream_set_frame_reduction(st._h, 2, fmt, pitch) == OK
        for fmt in (pnp.GRAY16_BE, *pnp.BAYER16_IDS):                     # ... and refused by a stream for the 2-byte ones
            assert ctx._lib.nmi_stream_set_frame_reduction(st._h, 2, fmt, 4 * W + 1) == E
            assert ctx._lib.nmi_stream_set_frame_reduction(st._h, 2, fmt, 4 * W + 2) == OK
        ctx.synchronize()


def test_bayer16_needs_two_by_two(nmi):
    src = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    for w, h in ((1, 2), (2, 1), (1, 1)):
        out = Outputs(w, h)
        with nmi.NmiContext(w, h) as ctx:
            for fmt in pnp.BAYER16_IDS:
                assert set(every_entry(ctx, src.data_ptr(), fmt, 0, 1, out)) == {E}
                assert set(every_entry(ctx, src.data_ptr(), fmt, 0, 2, out)) == {OK}       # 2 x 4, 4 x 2, 2 x 2 sites
                assert set(every_entry(ctx, src.data_ptr(), pnp.GRAY16_BE, 0, 1, out)) == {OK}
            ctx.synchronize()


def test_unpack_takes_the_nine_formats_only(nmi):
    src = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    out = Outputs(W, H)
    with nmi.NmiContext(W, H) as ctx, nmi.NmiStream(ctx, 2, 2) as st:
        lib, h = ctx._lib, ctx._h
        for fmt in [capi.FRAME_GRAY16, *EIGHT_BIT, *UNKNOWN]:
            for f in (1, 2):
                assert lib.nmi_unpack_frame(h, src.data_ptr(), fmt, 0, f, out.cont.data_ptr()) == E, fmt
        for fmt in UNKNOWN:                                                # unknown everywhere a format is taken
            assert lib.nmi_gray_frame(h, src.data_ptr(), fmt, 0, out.gray.data_ptr()) == E, fmt
            assert lib.nmi_reduce_frame(h, src.data_ptr(), fmt, 0, 2, None, out.gray.data_ptr(), None) == E, fmt
            assert lib.nmi_stream_set_frame_format(st._h, fmt, 0) == E, fmt
            assert lib.nmi_stream_set_frame_reduction(st._h, 2, fmt, 0) == E, fmt
            assert lib.nmi_level_set_frame_format(None, fmt, 0) == E and lib.nmi_frame_row_bytes(fmt, 8) == 0
        ctx.synchronize()
        assert out.untouched()
        with pytest.raises(capi.NmiError):
            ctx.unpack_frame(src, capi.FRAME_GRAY16)

        def room(n):
            return torch.zeros(n, dtype=torch.uint8, device="cuda")

        with pytest.raises(ValueError):                                    # the wrapper's own check of the source's size
            ctx.unpack_frame(room(pnp.span(pnp.MONO12P, W, H) - 1), pnp.MONO12P)
        with pytest.raises(ValueError):
            ctx.reduce_frame(room(pnp.span(pnp.RAW10, 2 * W, 2 * H, 61) - 1), pnp.RAW10, 2, 61)
        assert ctx.unpack_frame(room(pnp.span(pnp.MONO12P, W, H)), pnp.MONO12P).shape == (H, W)
        assert ctx.reduce_frame(room(pnp.span(pnp.RAW10, 2 * W, 2 * H, 61)), pnp.RAW10, 2, 61).shape == (H, W)
