"""GPU tests (-m gpu) of what the deep grey frames (NMI_FRAME_GRAY16, nmi_tone_map) refuse: every rejection is
NMI_ERR_INVALID_ARGUMENT before anything is enqueued, with the output untouched and the setting as it was; the neighbouring ids
stay unknown, and a tone map changes nothing for the other formats."""
import ctypes as C

import numpy as np
import pytest

from helpers import color_np as cnp
from helpers import sensor_np as snp
from helpers import tone_np as tnp
from orbslam2_nmi_amd import capi

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

W, H = 64, 48
E = capi.ERR_INVALID_ARGUMENT
G16 = capi.FRAME_GRAY16
C_INT5 = C.c_int32 * 5


@pytest.fixture(scope="module")
def nmi():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    import orbslam2_nmi_amd as m
    m.load_library()
    return m


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bad_tone_maps(d_lut):
    T = capi.ToneMap
    return {
        "bits 7": T(mode=capi.TONE_SHIFT, bits=7), "bits 17": T(mode=capi.TONE_SHIFT, bits=17),
        "lo == hi": T(mode=capi.TONE_WINDOW, bits=12, lo=100, hi=100), "lo > hi": T(mode=capi.TONE_WINDOW, bits=12, lo=200, hi=100),
        "lo < 0": T(mode=capi.TONE_WINDOW, bits=12, lo=-1, hi=100), "hi > M": T(mode=capi.TONE_WINDOW, bits=12, lo=0, hi=4096),
        "p_lo < 0": T(mode=capi.TONE_PERCENTILE, bits=16, p_lo=-1, p_hi=0), "p_hi < 0": T(mode=capi.TONE_PERCENTILE, bits=16, p_lo=0, p_hi=-5),
        "shares 10000": T(mode=capi.TONE_PERCENTILE, bits=16, p_lo=4000, p_hi=6000),
        "plateau < 0": T(mode=capi.TONE_EQUALIZE, bits=16, plateau=-1),
        "reserved": T(mode=capi.TONE_SHIFT, bits=16, reserved=(C_INT5(0, 0, 0, 0, 1))),
        "reserved first": T(mode=capi.TONE_EQUALIZE, bits=16, reserved=(C_INT5(7, 0, 0, 0, 0))),
        "table NULL": T(mode=capi.TONE_TABLE, bits=16),
        "mode 5": T(mode=5, bits=16), "mode -1": T(mode=-1, bits=16),
        "table, bits 20": T(mode=capi.TONE_TABLE, bits=20, d_lut=d_lut.data_ptr()),
    }


def test_frame_rejections_leave_the_output(nmi):
    out = torch.full((H, W), 0xAB, dtype=torch.uint8, device="cuda")
    small = torch.full((H // 2, W // 2), 0xAB, dtype=torch.uint8, device="cuda")
    src = torch.zeros(H * W * 2 + 4096, dtype=torch.uint8, device="cuda")
    lut = torch.full((tnp.LEVELS,), 0xAB, dtype=torch.uint8, device="cuda")
    sp, op = src.data_ptr(), out.data_ptr()
    with nmi.NmiContext(W, H) as ctx, nmi.NmiContext(W // 2, H // 2) as half:
        lib, h = ctx._lib, ctx._h
        ctx.set_tone_map(capi.ToneMap.equalize())                     # (a mode with nodes to enqueue)
        half.set_tone_map(capi.ToneMap.equalize())
        assert lib.nmi_gray_frame(h, sp + 1, G16, 0, op) == E          # an odd base
        assert lib.nmi_gray_frame(h, sp + 3, G16, 2 * W + 2, op) == E
        for pitch in (2 * W + 1, 2 * W + 63, 1, W, 2 * W - 2, 2 * W - 1, -2 * W):   # an odd pitch, pitch < 2 W
            assert lib.nmi_gray_frame(h, sp, G16, pitch, op) == E, pitch
        # d_gray overlapping the source: its first byte, its last byte, inside a pitched frame's padding
        assert lib.nmi_gray_frame(h, sp, G16, 0, sp) == E
        assert lib.nmi_gray_frame(h, sp + 4000, G16, 0, sp + 4000 - H * W + 1) == E
        assert lib.nmi_gray_frame(h, sp, G16, 0, sp + 2 * H * W - 1) == E
        assert lib.nmi_gray_frame(h, sp, G16, 2 * W + 16, sp + 2 * W + 2) == E
        for fmt in (47, 49):                                           # the neighbouring ids stay unknown
            assert lib.nmi_gray_frame(h, sp, fmt, 0, op) == E
            assert lib.nmi_reduce_frame(half._h, sp, fmt, 0, 2, None, small.data_ptr(), None) == E
        # the same through nmi_reduce_frame (a 32x24 context at factor 2 reads the 64x48 source) and nmi_tone_lut
        hp, smp = half._h, small.data_ptr()
        assert lib.nmi_reduce_frame(hp, sp + 1, G16, 0, 2, None, smp, None) == E
        assert lib.nmi_reduce_frame(hp, sp, G16, 2 * W + 1, 2, None, smp, None) == E
        assert lib.nmi_reduce_frame(hp, sp, G16, 2 * W - 2, 2, None, smp, None) == E
        assert lib.nmi_reduce_frame(hp, sp, G16, 0, 2, None, sp + 2 * H * W - 1, None) == E
        assert lib.nmi_reduce_frame(hp, sp, G16, 0, 5, None, smp, None) == E
        lp = lut.data_ptr()
        assert lib.nmi_tone_lut(h, sp + 1, 0, 1, lp, None) == E
        assert lib.nmi_tone_lut(h, sp, 2 * W + 1, 1, lp, None) == E
        assert lib.nmi_tone_lut(h, sp, 2 * W - 2, 1, lp, None) == E
        assert lib.nmi_tone_lut(h, sp, 0, 0, lp, None) == E
        assert lib.nmi_tone_lut(h, sp, 0, 5, lp, None) == E
        assert lib.nmi_tone_lut(h, sp, 0, 1, sp + 2 * H * W - 1, None) == E
        assert lib.nmi_tone_lut(h, sp, 0, 1, None, None) == E
        # just outside: accepted (the grey frame ends where the source begins)
        g = torch.zeros(H * W + H * W * 2, dtype=torch.uint8, device="cuda")
        assert lib.nmi_gray_frame(h, g.data_ptr() + H * W, G16, 0, g.data_ptr()) == capi.NMI_OK
        ctx.synchronize()
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 0xAB).all() and (small.cpu().numpy() == 0xAB).all() and (lut.cpu().numpy() == 0xAB).all()


def test_a_bad_source_is_refused_before_the_mode_is(nmi):
    """nmi_tone_lut under CLAHE and nmi_tone_tile_luts under any other mode answer NMI_ERR_UNSUPPORTED -- for good arguments
    only: a bad source, factor or table pointer is NMI_ERR_INVALID_ARGUMENT under every mode."""
    w, h = 8, 8
    src = torch.zeros(w * h * 2 + 64, dtype=torch.uint8, device="cuda")
    lut = torch.full((tnp.LEVELS,), 0xAB, dtype=torch.uint8, device="cuda")
    sp, lp = src.data_ptr(), lut.data_ptr()
    with nmi.NmiContext(w, h) as ctx:
        lib, hd = ctx._lib, ctx._h
        for tm, entry in ((capi.ToneMap.clahe(1, 1, plateau=0, bits=12), lib.nmi_tone_lut), (capi.ToneMap.equalize(bits=12), lib.nmi_tone_tile_luts),
                          (None, lib.nmi_tone_tile_luts)):
            ctx.set_tone_map(tm)
            assert entry(hd, sp, 0, 1, lp, None) == capi.ERR_UNSUPPORTED
            assert entry(hd, sp + 1, 0, 1, lp, None) == E                  # an odd base
            assert entry(hd, sp, 2 * w + 1, 1, lp, None) == E              # an odd pitch
            assert entry(hd, sp, 2 * w - 2, 1, lp, None) == E              # a pitch below the row
            assert entry(hd, sp, 0, 0, lp, None) == E and entry(hd, sp, 0, 5, lp, None) == E
            assert entry(hd, None, 0, 1, lp, None) == E and entry(hd, sp, 0, 1, None, None) == E
            assert entry(hd, sp, 0, 1, sp + 2 * w * h - 1, None) == E      # the table meets the source's last byte
        ctx.synchronize()
    torch.cuda.synchronize()
    assert (lut.cpu().numpy() == 0xAB).all()


def test_bad_tone_maps_leave_the_setting(nmi):
    px = tnp.thermal(W, H, 4)
    d = dev(tnp.pack16(px))
    d_lut = torch.zeros(tnp.LEVELS, dtype=torch.uint8, device="cuda")
    good = tnp.tone(tnp.PERCENTILE, 14, p_lo=50, p_hi=50)
    want = tnp.apply(px, good)
    out = torch.full((H, W), 0xAB, dtype=torch.uint8, device="cuda")
    with nmi.NmiContext(W, H) as ctx, nmi.NmiStream(ctx, 2, 2) as st:
        ctx.set_tone_map(tnp.capi_tone(capi, good))
        for name, tm in bad_tone_maps(d_lut).items():
            assert ctx._lib.nmi_set_tone_map(ctx._h, C.byref(tm)) == E, name
            assert ctx._lib.nmi_stream_set_tone_map(st._h, C.byref(tm)) == E, name
            assert ctx._lib.nmi_level_set_tone_map(None, C.byref(tm)) == E, name
        assert (out.cpu().numpy() == 0xAB).all()
        assert ctx._lib.nmi_set_tone_map(None, None) == E and ctx._lib.nmi_tone_map_default(None) == E
        assert (ctx.gray_frame(d, G16).cpu().numpy() == want).all()    # the setting is the good one still


def test_a_tone_map_changes_no_other_format(nmi):
    rgb = snp.chroma_frame(W, H, seed=3)
    sources = {cnp.BGR: cnp.pack(rgb, cnp.BGR, 0, seed=1), snp.YUYV: snp.pack(rgb[..., 1].copy(), snp.YUYV, seed=2),
               snp.GRBG: snp.pack(snp.mosaic(rgb, snp.GRBG), snp.GRBG), cnp.GRAY: rgb[..., 0].copy().reshape(-1)}
    with nmi.NmiContext(W, H) as ctx:
        before = {f: ctx.gray_frame(dev(b), f).cpu().numpy() for f, b in sources.items()}
        assert (before[cnp.BGR] == cnp.to_gray(sources[cnp.BGR], cnp.BGR, W, H)).all()
        assert (before[snp.GRBG] == snp.to_gray(sources[snp.GRBG], snp.GRBG, W, H)).all()
        for tm in (capi.ToneMap.equalize(plateau=3), capi.ToneMap.window(3, 9, bits=8), capi.ToneMap.percentile(100, 100)):
            ctx.set_tone_map(tm)
            for f, b in sources.items():
                assert (ctx.gray_frame(dev(b), f).cpu().numpy() == before[f]).all(), f
