"""GPU tests (-m gpu) of captured levels and keyframe streams fed raw sensor frames (NMI_FRAME_YUYV / _UYVY / _BAYER_*, through
nmi_level_set_frame_format / _set_frame_reduction and their nmi_stream_* twins), at 64x48 with S = 3, Wn = 3.

Levels: a replay equals the standalone chain on the twin's grey frame (tests/helpers/sensor_np.py) -- nmi_gray_frame or
nmi_reduce_frame (== the twin) -> [nmi_undistort_frame(_fisheye)] -> warps -> search -- on == of winner, score bits, warps, warp
masks and coverage (the harness of tests/test_reduce_level.py).  Streams: tickets on raw host frames equal the tickets of a
stream with the same lens fed the twin's grey frames (the harness of tests/test_color_stream.py), which tests/test_stream_*.py
tie to the standalone calls; and a stream that changes between 3-, 1- and 2-byte formats and sizes keeps doing so."""
import numpy as np
import pytest

from helpers import color_np as cnp
from helpers import fisheye_np as fnp
from helpers import sensor_np as snp
from helpers import undistort_np as unp
from orbslam2_nmi_amd import synthetic as sy
from test_color_level import bits, enable, lens_K, scene
from test_color_stream import outcome, same, submit
from test_fisheye_level import raw_K
from test_masked_level import dev, hood_mask, views, warps
from test_reduce_level import check_against, full_size
from test_stream_masked import hood, level, pin, render_masks

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

W, H, S, WN = 64, 48, 3, 3
RADTAN = unp.FAMILIES["barrel"]
FISHEYE = fnp.FAMILIES["euroc_eq"]
# kind, lens, factor: plain; masked with radial-tangential distortion; covered with reduction 2 and a fisheye lens
CASES = {"plain": ("plain", None, 1), "masked-radtan": ("masked", "radtan", 1), "covered-f2-fisheye": ("covered", "fisheye", 2)}
# format, extra pitch bytes, base offset: a mosaic on the byte paths, packed YUV on the vector paths
LAYOUTS = {"grbg-pitched-offset": (snp.GRBG, 5, 3), "yuyv-aligned": (snp.YUYV, 16, 0)}


@pytest.fixture(scope="module")
def nmi():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    import orbslam2_nmi_amd as m
    m.load_library()
    return m


def raw_frame(gray, f, fmt, pitch, off=0, seed=0):
    """The search-size grey frame at f times its size, as a mosaic of its coloured form (Bayer) or as luma (YUV), laid out in fmt
    -> (flat buffer, the twin's grey frame of the search size)."""
    big = gray if f == 1 else full_size(gray, f, seed)
    img = snp.mosaic(cnp.colorize(big, seed), fmt) if snp.is_bayer(fmt) else big
    buf = snp.pack(img, fmt, pitch, off, seed=seed)
    h, w = gray.shape
    return buf, snp.reduce_frame(buf, fmt, w, h, f, pitch, off)


def lens_of(name, K, ctx):
    """-> (K_raw, coefficients, the context the chain's undistort_frame goes through)."""
    if name == "fisheye":
        Kr = raw_K(K, W)
        return Kr, FISHEYE, fnp.FisheyeCtx(ctx, Kr)
    return None, (RADTAN if name == "radtan" else None), ctx


def set_lens(target, name, K, Kr, dist):
    if name == "fisheye":
        target.set_distortion_fisheye(K, Kr, dist)
    elif name == "radtan":
        target.set_distortion(K, dist)


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("case", list(CASES))
def test_sensor_level_equals_the_chain(nmi, case, layout):
    kind, lens, f = CASES[case]
    fmt, extra, off = LAYOUTS[layout]
    pitch = f * W * snp.BPP[fmt] + extra
    with nmi.NmiContext(W, H) as ctx:
        sc = scene(nmi, ctx, W, H, False, kind)
        K = lens_K(sc.rp)
        Kr, dist, cctx = lens_of(lens, K, ctx)
        gray0 = sc.frame.cpu().numpy()
        buf, twin = raw_frame(gray0, f, fmt, pitch, off)
        d = dev(buf)
        fm = dev(hood_mask(W, H)) if kind != "plain" else None
        mvps, Ms = views(sc.rp, S), warps(W, H, WN)

        def chain_gray():
            g = ctx.reduce_frame(d[off:], fmt, f, pitch) if f > 1 else ctx.gray_frame(d[off:], fmt, pitch)
            assert (g.cpu().numpy() == twin).all()
            return g

        def make():
            return nmi.NmiLevel(sc.ctx, sc.dx, sc.da, d[off:], S, WN, 3.0, texture=sc.tex)

        with make() as lv, make() as lv2:
            lv.set_frame_reduction(f, fmt, pitch) if f > 1 else lv.set_frame_format(fmt, pitch)   # format, lens, masks
            set_lens(lv, lens, K, Kr, dist)
            enable(lv, kind, fm)
            enable(lv2, kind, fm)                                                                # masks, lens, format
            set_lens(lv2, lens, K, Kr, dist)
            lv2.set_frame_reduction(f, fmt, pitch)
            first = check_against(cctx, sc, chain_gray(), lv, kind, K, dist, fm, mvps, Ms)
            again = check_against(cctx, sc, chain_gray(), lv2, kind, K, dist, fm, mvps, Ms)
            assert again[0] == first[0] and (bits(again[1]) == bits(first[1])).all()
            buf, twin = raw_frame(np.roll(gray0, shift=(7, 11), axis=(0, 1)), f, fmt, pitch, off, seed=1)
            d.copy_(dev(buf))                                                                    # the frame changes in place
            torch.cuda.synchronize()
            moved = check_against(cctx, sc, chain_gray(), lv, kind, K, dist, fm, views(sc.rp, S, 1.7), warps(W, H, WN, 1.6))
            assert (bits(moved[1]) != bits(first[1])).any()
            for bad in ((1, 18, 0), (2, 36, 0), (1, fmt, 1), (1, snp.RGGB, W - 1), (1, snp.UYVY, 2 * W - 1)):
                with pytest.raises(nmi.capi.NmiError):
                    lv.set_frame_reduction(*bad)
            after = check_against(cctx, sc, chain_gray(), lv, kind, K, dist, fm, views(sc.rp, S, 1.7), warps(W, H, WN, 1.6))
            assert (bits(after[1]) == bits(moved[1])).all()                                      # as it was


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("case", list(CASES))
def test_sensor_tickets_equal_grey_tickets(nmi, case, layout):
    kind, lens, f = CASES[case]
    fmt, extra, _ = LAYOUTS[layout]
    pitch = f * W * snp.BPP[fmt] + extra
    K = sy.intrinsics(W, H)
    F, rs, Ms = level(W, H, (3, 1, 1), (3, 1, 1), seed=5)
    F2, rs2, _ = level(W, H, (3, 1, 1), (3, 1, 1), seed=9)
    assert (len(rs), len(Ms)) == (S, WN)
    fm = hood(W, H) if kind != "plain" else None
    rm = render_masks(S, W, H, 3) if kind == "covered" else None
    H1, G1 = raw_frame(F, f, fmt, pitch, seed=1)
    H2, G2 = raw_frame(F2, f, fmt, pitch, seed=2)
    assert G1.shape == (H, W) and (G1 != G2).any()
    with nmi.NmiContext(W, H) as ctx, nmi.NmiStream(ctx, S, WN, depth=4) as st, nmi.NmiStream(ctx, S, WN, depth=4) as ref:
        Kr, dist, _ = lens_of(lens, K, ctx)
        for s in (st, ref):
            s.keep_ratings()
            set_lens(s, lens, K, Kr, dist)
        t_before = submit(ctx, st, kind, rs, rm, pin(G1), fm, Ms, None)       # grey, submitted before the setting
        st.set_frame_reduction(f, fmt, pitch)
        t1 = submit(ctx, st, kind, rs, rm, pin(H1), fm, Ms, None)
        t2 = submit(ctx, st, kind, rs2, rm, None, None, Ms, None)            # frame-less: the latest warps
        t3 = submit(ctx, st, kind, rs, rm, pin(H2), fm, Ms, True)            # the block form
        r_before = submit(ctx, ref, kind, rs, rm, pin(G1), fm, Ms, None)
        r1 = submit(ctx, ref, kind, rs, rm, pin(G1), fm, Ms, None)
        r2 = submit(ctx, ref, kind, rs2, rm, None, None, Ms, None)
        r3 = submit(ctx, ref, kind, rs, rm, pin(G2), fm, Ms, True)
        for t, r in ((t_before, r_before), (t1, r1), (t2, r2), (t3, r3)):
            same(outcome(st, t, WN, S, kind), outcome(ref, r, WN, S, kind))
        st.set_frame_format(cnp.GRAY, 0)                                     # off: later frames are dense grey again
        t4 = submit(ctx, st, kind, rs, rm, pin(G2), fm, Ms, None)
        r4 = submit(ctx, ref, kind, rs, rm, pin(G2), fm, Ms, None)
        same(outcome(st, t4, WN, S, kind), outcome(ref, r4, WN, S, kind))


def test_a_stream_goes_from_rgb_to_bayer_and_back(nmi):
    """RGB -> Bayer -> RGB between tickets, then packed YUV at twice the size and back: the colour slots are sized for 3, 1 and 2
    bytes per pixel in turn, grow for the larger frame and keep serving the smaller ones."""
    F, rs, Ms = level(W, H, (3, 1, 1), (3, 1, 1), seed=3)
    F2, _, _ = level(W, H, (3, 1, 1), (3, 1, 1), seed=4)
    C = cnp.colorize(F, 4)
    rgb = cnp.pack(C, cnp.RGB, W * 3 + 1, seed=7)
    settings = [(1, cnp.RGB, W * 3 + 1), (1, snp.BGGR, 0), (1, cnp.RGB, W * 3 + 1), (2, snp.UYVY, 4 * W + 6), (1, snp.RGGB, W + 3),
                (3, snp.GBRG, 0), (1, cnp.RGB, W * 3 + 1)]
    with nmi.NmiContext(W, H) as ctx, nmi.NmiStream(ctx, S, WN, depth=2) as st, nmi.NmiStream(ctx, S, WN, depth=2) as ref:
        st.keep_ratings()
        ref.keep_ratings()
        seen = []
        for k, (f, fmt, pitch) in enumerate(settings):
            st.set_frame_reduction(f, fmt, pitch)
            for bad in ((f, 5, 0), (f, 31, 0), (f, fmt, 1)):
                with pytest.raises(nmi.capi.NmiError):
                    st.set_frame_reduction(*bad)
            src = F if k % 2 == 0 else F2
            if fmt == cnp.RGB:
                Hk, Gk = rgb, cnp.to_gray(rgb, cnp.RGB, W, H, pitch)
            else:
                Hk, Gk = raw_frame(src, f, fmt, pitch, seed=k)
            t = st.submit(pin(rs), pin(Hk), Ms)
            r = ref.submit(pin(rs), pin(Gk), Ms)
            same(outcome(st, t, WN, S, "plain"), outcome(ref, r, WN, S, "plain"))
            seen.append(bits(st.ratings(t, WN, S)).copy())
        assert (seen[0] == seen[2]).all() and (seen[0] == seen[6]).all() and (seen[0] != seen[1]).any()
