"""GPU tests (-m gpu) of what the valid-range entries refuse and keep (include/nmi_hip.h "Deep frames"): a bad range leaves the
setting as it was; every argument error of nmi_deep_frame leaves both outputs untouched; (0, 65535) after a range gives the
unranged bytes again; and the range is kept, and ignored, under NMI_FRAME_GRAY and a Bayer format."""
import numpy as np
import pytest

from helpers import clahe_np as cnp
from helpers import tone_np as tnp
from helpers import valid_cases as cases
from helpers import valid_np as vnp
from orbslam2_nmi_amd import capi

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

E = capi.ERR_INVALID_ARGUMENT
G16 = capi.FRAME_GRAY16
BAD_RANGES = [(-1, 100), (5, 4), (0, 65536), (65536, 65536), (-5, -1), (70000, 70001), (1, 0)]


@pytest.fixture(scope="module")
def nmi():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    import orbslam2_nmi_amd as m
    m.load_library()
    return m


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def test_a_bad_range_leaves_the_setting(nmi):
    w, h = 37, 23
    px, rng, bits = cases.frame("depth_holes", w, h, 1)
    tm = tnp.tone(tnp.EQUALIZE, bits)
    want = vnp.deep_frame(px, 1, tm, rng)
    with nmi.NmiContext(w, h) as ctx:
        ctx.set_tone_map(tnp.capi_tone(capi, tm))
        ctx.set_valid_range(*rng)
        lib = ctx._lib
        for lo, hi in BAD_RANGES:
            assert lib.nmi_set_valid_range(ctx._h, lo, hi) == E, (lo, hi)
        assert lib.nmi_set_valid_range(None, 1, 2) == E
        g, m = ctx.deep_frame(dev(tnp.pack16(px)))
        assert (g.cpu().numpy() == want[0]).all() and (m.cpu().numpy() == want[1]).all()
        for lo, hi in ((0, 0), (65535, 65535), (7, 7), (0, 65535)):                   # the edges of what is accepted
            ctx.set_valid_range(lo, hi)


def test_deep_frame_argument_errors_leave_the_outputs(nmi):
    w, h, f = 12, 8, 2
    ws, hs = f * w, f * h
    npix = w * h
    with nmi.NmiContext(w, h) as ctx:
        ctx.set_valid_range(1, 65535)
        lib, c = ctx._lib, ctx._h
        src = dev(tnp.pack16(tnp.uniform(ws, hs, seed=1), 2 * ws + 8))               # pitched: room for a frame mask inside it
        pitch = 2 * ws + 8
        pool = torch.full((4 * npix + 64,), 0xAB, dtype=torch.uint8, device="cuda")   # the frame mask and both outputs
        fm, gray, mask = pool.data_ptr(), pool.data_ptr() + npix + 16, pool.data_ptr() + 2 * npix + 32
        s = src.data_ptr()
        bad = {
            "NULL ctx": (None, s, pitch, f, fm, gray, mask), "NULL src": (c, None, pitch, f, fm, gray, mask),
            "NULL gray": (c, s, pitch, f, fm, None, mask), "NULL mask": (c, s, pitch, f, fm, gray, None),
            "factor 0": (c, s, pitch, 0, fm, gray, mask), "factor 5": (c, s, pitch, 5, fm, gray, mask),
            "odd src": (c, s + 1, pitch, f, fm, gray, mask), "odd pitch": (c, s, pitch + 1, f, fm, gray, mask),
            "negative pitch": (c, s, -pitch, f, fm, gray, mask), "short pitch": (c, s, 2 * ws - 2, f, fm, gray, mask),
            "gray == mask": (c, s, pitch, f, fm, gray, gray), "gray meets mask": (c, s, pitch, f, fm, gray, gray + npix - 1),
            "gray == frame mask": (c, s, pitch, f, fm, fm, mask), "mask == frame mask": (c, s, pitch, f, fm, gray, fm),
            "mask meets frame mask": (c, s, pitch, f, fm, gray, fm + npix - 1),
            "gray in the source": (c, s, pitch, f, fm, s + 2, mask), "mask in the source": (c, s, pitch, f, fm, gray, s + pitch),
            "mask at the source's last pixel": (c, s, pitch, f, fm, gray, s + (hs - 1) * pitch + 2 * ws - 1),
            "frame mask in the source": (c, s, pitch, f, s + 4, gray, mask),
            "gray before the source, reaching it": (c, s + 2 * npix, pitch, f, None, s + npix + 1, mask),
        }
        before = pool.clone()
        before_src = src.clone()
        for name, args in bad.items():
            assert lib.nmi_deep_frame(*args) == E, name
        ctx.synchronize()
        assert torch.equal(pool, before) and torch.equal(src, before_src)
        # touching is no overlap: the mask right behind the source's last pixel, the outputs back to back
        buf = torch.full((hs * pitch + 2 * npix,), 0xAB, dtype=torch.uint8, device="cuda")
        buf[:src.numel()] = src
        end = buf.data_ptr() + (hs - 1) * pitch + 2 * ws
        assert lib.nmi_deep_frame(c, buf.data_ptr(), pitch, f, None, end, end + npix) == 0
        ctx.synchronize()


def test_off_after_a_range_is_the_unranged_conversion(nmi):
    w, h = 40, 24
    px, rng, bits = cases.frame("depth_holes", w, h, 1)
    with nmi.NmiContext(w, h) as ctx:
        for tm in (tnp.tone(tnp.EQUALIZE, bits), tnp.tone(tnp.PERCENTILE, bits), cnp.clahe(3, 2, 2, bits)):
            unranged = cnp.apply(px, tm) if vnp.tiled(tm) else tnp.apply(px, tm)
            ranged = vnp.apply(px, tm, rng)
            assert (ranged != unranged).any()
            ctx.set_tone_map(cases.capi_tone(capi, tm))
            src = dev(tnp.pack16(px))
            seen = []
            for r in (vnp.OFF, rng, vnp.OFF, (1, 65534), (0, 65535)):
                ctx.set_valid_range(*r)
                seen.append(ctx.gray_frame(src, G16).cpu().numpy())
            assert (seen[0] == unranged).all() and (seen[2] == unranged).all() and (seen[4] == unranged).all()
            assert (seen[1] == ranged).all() and (seen[3] == vnp.apply(px, tm, (1, 65534))).all()
            g, m = ctx.deep_frame(src)                                                # range off: every pixel valid
            assert (g.cpu().numpy() == unranged).all() and (m.cpu().numpy() == 1).all()
            fm = (np.random.default_rng(2).random((h, w)) < 0.5).astype(np.uint8) * 200
            g, m = ctx.deep_frame(src, frame_mask=dev(fm))
            assert (g.cpu().numpy() == unranged).all() and (m.cpu().numpy() == (fm != 0)).all()


@pytest.mark.parametrize("fmt", ["FRAME_GRAY", "FRAME_BAYER_RGGB"])
def test_the_range_is_kept_and_ignored_under_other_formats(nmi, fmt):
    w, h = 40, 24
    fmt = getattr(capi, fmt)
    px, rng, bits = cases.frame("depth_holes", w, h, 1)
    tm = tnp.tone(tnp.EQUALIZE, bits)
    eight = np.random.default_rng(3).integers(0, 256, (2 * h, 2 * w + 4)).astype(np.uint8)
    eight[::3, ::5] = 0                                                               # values a range (1, ...) would call invalid
    sm = (np.random.default_rng(4).random((2 * h, 2 * w)) < 0.9).astype(np.uint8)
    with nmi.NmiContext(w, h) as ctx:
        ctx.set_tone_map(tnp.capi_tone(capi, tm))
        src8 = dev(eight)
        off = [ctx.gray_frame(src8, fmt, 2 * w + 4).cpu().numpy()]
        off += [t.cpu().numpy() for t in ctx.reduce_frame(src8, fmt, 2, 2 * w + 4, src_mask=dev(sm))]
        ctx.set_valid_range(*rng)
        on = [ctx.gray_frame(src8, fmt, 2 * w + 4).cpu().numpy()]
        on += [t.cpu().numpy() for t in ctx.reduce_frame(src8, fmt, 2, 2 * w + 4, src_mask=dev(sm))]
        for a, b in zip(off, on):
            assert (a == b).all()
        g, m = ctx.deep_frame(dev(tnp.pack16(px)))                                    # kept: the next deep frame is ranged
        want = vnp.deep_frame(px, 1, tm, rng)
        assert (g.cpu().numpy() == want[0]).all() and (m.cpu().numpy() == want[1]).all()
