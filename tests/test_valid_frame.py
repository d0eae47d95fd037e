"""GPU tests (-m gpu) of the valid range of deep grey frames (nmi_set_valid_range, include/nmi_hip.h "Deep frames") on the
standalone entries: nmi_deep_frame, nmi_gray_frame, nmi_reduce_frame, nmi_tone_lut (with h_window) and nmi_tone_tile_luts (with
h_counts) == the numpy twin (tests/helpers/valid_np.py), byte for byte.  Contexts of 40 x 24 and 37 x 23 (the conversion's last
quad and the histogram's last run partial), factors 1 .. 4, bits 12, 14 and 16, every mode and CLAHE at 1 x 1, 3 x 2 and 8 x 8
tiles, dense / pitched / 2 bytes off 16-byte alignment, on the planted frames of tests/helpers/valid_cases.py (whose premises --
the range changes the table, the mask has both values -- tests/test_valid_twin.py checks)."""
import numpy as np
import pytest

from helpers import reduce_np as rnp
from helpers import tone_np as tnp
from helpers import valid_cases as cases
from helpers import valid_np as vnp
from orbslam2_nmi_amd import capi

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

G16 = capi.FRAME_GRAY16


@pytest.fixture(scope="module")
def nmi():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    import orbslam2_nmi_amd as m
    m.load_library()
    return m


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def fresh(h, w, shift=0):
    """A [h,w] uint8 device image of 0xAB bytes, its first byte `shift` bytes into a 16-byte aligned allocation."""
    return torch.full((h * w + 16,), 0xAB, dtype=torch.uint8, device="cuda")[shift:shift + h * w].view(h, w)


def same(got, want, what):
    got = got.cpu().numpy() if hasattr(got, "cpu") else np.asarray(got)
    assert got.shape == want.shape and (got == want).all(), (what, np.argwhere(got != want)[:5])


def set_tone(ctx, tm, keep):
    d_lut = None
    if tm["mode"] == tnp.TABLE:
        d_lut = dev(tm["lut"])
        keep.append(d_lut)
    ctx.set_tone_map(cases.capi_tone(capi, tm, d_lut))


def every_entry_equals_the_twin(nmi, name, size, factors, frame=cases.frame):
    """Every entry on the planted frame frame(name, w, h, f) of a w x h context, at every factor, tone map and layout."""
    w, h = size
    keep = []
    fm = (np.random.default_rng(11).random((h, w)) < 0.85).astype(np.uint8) * 5          # a frame mask at the search size
    with nmi.NmiContext(w, h) as ctx:
        for f in factors:
            ws, hs = f * w, f * h
            px, rng, bits = frame(name, w, h, f)
            sm = (np.random.default_rng(12 + f).random((hs, ws)) < 0.95).astype(np.uint8) * 9  # nmi_reduce_frame's own, full size
            ctx.set_valid_range(*rng)
            for tm in cases.tone_maps(bits, ws, hs):
                what = (name, size, f, tm["label"])
                set_tone(ctx, tm, keep)
                want_gray, want_mask = vnp.deep_frame(px, f, tm, rng)
                want_mask_fm = vnp.mask(px, f, rng, fm)
                want_pair = rnp.reduce_mask(sm, f) & vnp.mask(px, f, rng)
                for li, (extra, off) in enumerate(cases.LAYOUTS):
                    pitch, off = cases.layout(ws, extra, off)
                    src = dev(tnp.pack16(px, pitch, off, seed=li))[off:]
                    shift = li % 2                                                     # (odd: outputs off 4-byte alignment)
                    g, m = ctx.deep_frame(src, f, pitch, out=fresh(h, w, shift), out_mask=fresh(h, w, shift))
                    same(g, want_gray, what + ("deep", li))
                    same(m, want_mask, what + ("deep mask", li))
                    g, m = ctx.deep_frame(src, f, pitch, frame_mask=dev(fm), out=fresh(h, w), out_mask=fresh(h, w, 2 * shift))
                    same(g, want_gray, what + ("deep + frame mask", li))
                    same(m, want_mask_fm, what + ("deep mask + frame mask", li))
                    if f == 1:
                        same(ctx.gray_frame(src, G16, pitch, out=fresh(h, w)), want_gray, what + ("gray", li))
                    same(ctx.reduce_frame(src, G16, f, pitch, out=fresh(h, w)), want_gray, what + ("reduce", li))
                    g, m = ctx.reduce_frame(src, G16, f, pitch, src_mask=dev(sm), out=fresh(h, w), out_mask=fresh(h, w))
                    same(g, want_gray, what + ("reduce + masks", li))
                    same(m, want_pair, what + ("reduce mask", li))
                    if vnp.tiled(tm):
                        luts, n = ctx.tone_tile_luts(src, f, pitch)
                        want_luts, want_n = vnp.tile_luts(px, tm, rng)
                        same(luts, want_luts, what + ("tile luts", li))
                        assert (n == want_n).all(), what
                    else:
                        lut, pair = ctx.tone_lut(src, f, pitch)
                        want_lut, want_window = vnp.table(px, tm, rng)
                        same(lut, want_lut, what + ("lut", li))
                        assert tuple(pair) == tuple(int(x) for x in want_window), (what, pair, want_window)


@pytest.mark.parametrize("size", cases.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", list(cases.FRAMES))
def test_every_entry_equals_the_twin(nmi, name, size):
    every_entry_equals_the_twin(nmi, name, size, cases.FRAMES[name]["factors"])


def test_the_next_frame_starts_from_clean_histograms(nmi):
    """A ranged frame, a frame with no valid pixel, the first again, under EQUALIZE at 16 bits and CLAHE: the (tile) histograms
    were left all zero, whatever was counted."""
    w, h = 37, 23
    a, rng_a, _ = cases.frame("wide_holes", w, h, 1)
    b, rng_b, _ = cases.frame("nothing_valid", w, h, 1)
    from helpers import clahe_np as cnp
    with nmi.NmiContext(w, h) as ctx:
        for tm in (tnp.tone(tnp.EQUALIZE, 16), cnp.clahe(3, 2, 1, 16)):
            ctx.set_tone_map(cases.capi_tone(capi, tm))
            for px, rng in ((a, rng_a), (b, rng_b), (a, rng_a), (a, vnp.OFF), (a, rng_a)):
                ctx.set_valid_range(*rng)
                g, m = ctx.deep_frame(dev(tnp.pack16(px)), out=fresh(h, w), out_mask=fresh(h, w))
                want_gray, want_mask = vnp.deep_frame(px, 1, tm, rng)
                same(g, want_gray, (tm["mode"], rng))
                same(m, want_mask, (tm["mode"], rng, "mask"))
