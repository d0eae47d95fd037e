"""GPU tests (-m gpu) of nmi_undistort_frame_fisheye (csrc/nmi_undistort.hip): frame bytes and mask bytes == the numpy twin
(tests/helpers/fisheye_np.py) for every coefficient family, focal scale, frame size (dword and byte stores) and raw mask;
K_raw = NULL is K; the radial-tangential instantiation still gives its twin's bytes; the float64 tie-distance criterion of
tests/test_warp_edges.py on a smooth frame; and the fused colour node of a level against nmi_gray_frame followed by
nmi_undistort_frame_fisheye."""
import numpy as np
import pytest

from helpers import color_np as cnp
from helpers import fisheye_np as fnp
from helpers import undistort_np as unp
from orbslam2_nmi_amd import synthetic as sy
from test_warp_edges import RHO, noisy_frame, smooth_frame, tap_range

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SIZES = [(640, 480), (1241, 376), (333, 97), (17, 5), (3, 2), (1, 1)]


@pytest.fixture(scope="module")
def nmi():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    import orbslam2_nmi_amd as m
    m.load_library()
    return m


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def raw_masks(W, H):
    rng = np.random.default_rng(W * 7 + H)
    return {"none": None, "random": (rng.random((H, W)) < 0.9).astype(np.uint8), "zero": np.zeros((H, W), np.uint8)}


@pytest.mark.parametrize("scale", [1.0, 0.35])
@pytest.mark.parametrize("shape", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_fisheye_equals_the_twin(nmi, shape, scale):
    W, H = shape
    Kr = fnp.raw_K(W, H)
    K = fnp.pinhole_K(Kr, scale)
    img = noisy_frame(W, H)
    with nmi.NmiContext(W, H) as ctx:
        raw = dev(img)
        for fam, coeffs in fnp.FAMILIES.items():
            xs, ys = fnp.source_coords((H, W), K, Kr, coeffs)
            ef = unp.sample(img, xs, ys)
            for mname, rm in raw_masks(W, H).items():
                f, m = ctx.undistort_frame_fisheye(raw, K, Kr, coeffs, raw_mask=None if rm is None else dev(rm))
                em = unp.valid((H, W), xs, ys, rm)
                assert (f.cpu().numpy() == ef).all(), (fam, mname, int((f.cpu().numpy() != ef).sum()))
                assert (m.cpu().numpy() == em).all(), (fam, mname, int((m.cpu().numpy() != em).sum()))
                if mname == "zero":
                    assert not m.cpu().numpy().any()
            # without an output mask: the same frame bytes
            f2, none = ctx.undistort_frame_fisheye(raw, K, Kr, coeffs, out_mask=False)
            assert none is None and (f2.cpu().numpy() == ef).all()
        if W * H > 1000 and scale < 1:
            _, m = ctx.undistort_frame_fisheye(raw, K, Kr, fnp.FAMILIES["tumvi"])
            assert 0 < m.cpu().numpy().sum() < W * H  # (the premise: a wider pinhole view leaves an invalid border)


@pytest.mark.parametrize("shape", [(640, 480), (333, 97), (1, 1)], ids=["640x480", "333x97", "1x1"])
def test_K_raw_null_is_K(nmi, shape):
    W, H = shape
    K = fnp.raw_K(W, H)
    img = noisy_frame(W, H)
    rm = raw_masks(W, H)["random"]
    with nmi.NmiContext(W, H) as ctx:
        a = ctx.undistort_frame_fisheye(dev(img), K, None, fnp.FAMILIES["strong"], raw_mask=dev(rm))
        b = ctx.undistort_frame_fisheye(dev(img), K, K, fnp.FAMILIES["strong"], raw_mask=dev(rm))
        ef, em = fnp.undistort(img, K, None, fnp.FAMILIES["strong"], rm)
        for got in (a, b):
            assert (got[0].cpu().numpy() == ef).all() and (got[1].cpu().numpy() == em).all()
        if W * H > 1000:
            assert (ef != img).any()   # no identity case: even the plain equidistant lens moves pixels
            z, _ = ctx.undistort_frame_fisheye(dev(img), K, None, fnp.FAMILIES["zero"])
            assert (z.cpu().numpy() != img).any()


def test_odd_output_offsets_take_the_byte_path(nmi):
    """Output rows that do not start on 4-byte boundaries (a frame at an odd offset of a larger buffer): the same bytes, and the
    bytes around them untouched."""
    W, H = 64, 16
    Kr = fnp.raw_K(W, H)
    K = fnp.pinhole_K(Kr, 0.5)
    img = noisy_frame(W, H)
    with nmi.NmiContext(W, H) as ctx:
        big = torch.zeros(W * H + 8, dtype=torch.uint8, device="cuda")
        bigm = torch.zeros(W * H + 8, dtype=torch.uint8, device="cuda")
        out, outm = big[3:3 + W * H].view(H, W), bigm[1:1 + W * H].view(H, W)
        ctx.undistort_frame_fisheye(dev(img), K, Kr, fnp.FAMILIES["strong"], out=out, out_mask=outm)
        ef, em = fnp.undistort(img, K, Kr, fnp.FAMILIES["strong"])
        assert ef.any() and em.any()
        assert (out.cpu().numpy() == ef).all() and (outm.cpu().numpy() == em).all()
        assert not big[:3].any() and not big[3 + W * H:].any() and not bigm[:1].any() and not bigm[1 + W * H:].any()


def test_radial_tangential_bytes_unchanged(nmi):
    """The model is a template parameter: the radial-tangential instantiation still equals its own twin."""
    W, H = 333, 97
    K = sy.intrinsics(W, H)
    img = noisy_frame(W, H)
    rm = raw_masks(W, H)["random"]
    with nmi.NmiContext(W, H) as ctx:
        f, m = ctx.undistort_frame(dev(img), K, unp.FAMILIES["strong_k3"], raw_mask=dev(rm))
        ef, em = unp.undistort(img, K, unp.FAMILIES["strong_k3"], rm)
        assert (f.cpu().numpy() == ef).all() and (m.cpu().numpy() == em).all()


@pytest.mark.parametrize("scale", [1.0, 0.5])
@pytest.mark.parametrize("family", ["zero", "tumvi", "euroc_eq", "strong"])
@pytest.mark.parametrize("shape", [(640, 480), (848, 480), (333, 97)], ids=["640x480", "848x480", "333x97"])
def test_float64_criterion(nmi, shape, family, scale):
    """At every pixel whose float64 value lies more than tau(p) = R(p) RHO + 2^-12 from a rounding tie the product's byte is
    the rounded float64 value; elsewhere within 1; fewer than 1 % of the inner pixels are that close to a tie."""
    W, H = shape
    Kr = fnp.raw_K(W, H)
    K = fnp.pinhole_K(Kr, scale)
    img = smooth_frame(W, H)
    coeffs = fnp.FAMILIES[family]
    with nmi.NmiContext(W, H) as ctx:
        got = ctx.undistort_frame_fisheye(dev(img), K, Kr, coeffs, out_mask=False)[0].cpu().numpy()
    val = fnp.undistort_value_f64(img, K, Kr, coeffs)
    ref = np.clip(np.rint(val), 0, 255).astype(int)
    u, v = fnp.source_coords_f64((H, W), K, Kr, coeffs)
    r, inner = tap_range(img, u, v)
    tau = r * RHO + 2.0 ** -12
    near = np.abs(val - np.floor(val) - 0.5) <= tau
    d = got.astype(int) - ref
    n_in = int(inner.sum())
    print(f"{W}x{H} {family} {scale}: near a tie {(near & inner).sum()} of {n_in} inner, far disagreements {(d[~near] != 0).sum()}")
    assert np.abs(d).max() <= 1
    assert (d[~near] == 0).all(), int((d[~near] != 0).sum())
    assert n_in < 1000 or (near & inner).sum() < 0.01 * n_in


@pytest.mark.parametrize("kind", ["plain", "masked"])
@pytest.mark.parametrize("case", [(333, 97, cnp.BGR, 0, 0), (640, 480, cnp.BGR, 0, 0), (333, 97, cnp.RGBA, 333 * 4 + 5, 3),
                                  (640, 480, cnp.RGBA, 640 * 4 + 16, 0)],
                         ids=["333x97-bgr", "640x480-bgr", "333x97-rgba-pitched", "640x480-rgba-pitched"])
def test_fused_colour_node(nmi, case, kind):
    """A level on a colour or pitched frame with the fisheye lens set (one node converts and undistorts) gives the bytes of
    nmi_gray_frame followed by nmi_undistort_frame_fisheye: warps, warp masks, ratings bits, winner."""
    from test_color_level import ColorFrame, check, enable, lens_K, level
    from test_masked_level import Scene, hood_mask, views, warps
    w, h, fmt, pitch, off = case
    S, Wn = 3, 3
    with nmi.NmiContext(w, h) as ctx:
        sc = Scene(nmi, ctx, w, h, False)
        K = lens_K(sc.rp)
        Kr = fnp.pinhole_K(K, 1 / 0.6)
        Kr[0, 2] += 0.02 * w
        coeffs = fnp.FAMILIES["euroc_eq"]
        cf = ColorFrame(sc, fmt, pitch, off)
        fm = dev(hood_mask(w, h)) if kind == "masked" else None
        mvps, Ms = views(sc.rp, S), warps(w, h, Wn)
        fctx = fnp.FisheyeCtx(ctx, Kr)
        with level(nmi, sc, cf, S, Wn) as lv, level(nmi, sc, cf, S, Wn) as lv2:
            lv.set_frame_format(fmt, pitch)            # format first, then the lens and the masks
            lv.set_distortion_fisheye(K, Kr, coeffs)
            enable(lv, kind, fm)
            enable(lv2, kind, fm)
            lv2.set_distortion_fisheye(K, Kr, coeffs)
            lv2.set_frame_format(fmt, pitch)
            first = check(fctx, sc, cf, lv, kind, K, coeffs, fm, mvps, Ms)
            again = check(fctx, sc, cf, lv2, kind, K, coeffs, fm, mvps, Ms)
            assert again[0] == first[0] and (again[1].view(np.uint32) == first[1].view(np.uint32)).all()
            # the standalone chain's frame really is the twin's (grey of the colour frame, then the fisheye twin)
            gray = ctx.gray_frame(cf.view, cf.fmt, cf.pitch)
            ud, udm = ctx.undistort_frame_fisheye(gray, K, Kr, coeffs)
            ef, em = fnp.undistort(gray.cpu().numpy(), K, Kr, coeffs)
            assert (ud.cpu().numpy() == ef).all() and (udm.cpu().numpy() == em).all() and 0 < em.sum() < w * h
