"""CPU checks of the fisheye boundary (include/nmi_hip.h: nmi_undistort_frame_fisheye, nmi_level_set_distortion_fisheye,
nmi_stream_set_distortion_fisheye; include/nmi_host.h: nmi_config_parse_lens / _load_lens) and of the numpy twin
(tests/helpers/fisheye_np.py) against the float64 model.  No device needed: every call below is rejected before anything
touches a device."""
import ctypes as C
import glob
import math
import os

import numpy as np
import pytest

from conftest import ROOT
from helpers import fisheye_np as fnp
from orbslam2_nmi_amd import build as nmi_build
from orbslam2_nmi_amd import capi, hostapi
from test_undistort_api import bad_Ks, dbl, flt
from test_warp_edges import RHO

FISHEYE = ("nmi_undistort_frame_fisheye", "nmi_level_set_distortion_fisheye", "nmi_stream_set_distortion_fisheye")
SIZES = [(640, 480), (848, 480), (1248, 376), (1241, 376), (333, 97)]


@pytest.fixture(scope="module")
def lib():
    nmi_build.build()
    return capi.load_library()


def test_fisheye_symbols_declared_bound_exported(lib):
    from test_capi_symbols import declared_symbols
    raw = C.CDLL(capi.library_path())
    for name in FISHEYE:
        assert name in declared_symbols(), name
        assert name in capi.EXPORTED_SYMBOLS, name
        assert hasattr(raw, name), f"libnmi_hip.so does not export {name}"
        assert getattr(lib, name).argtypes, f"{name} has no argtypes"
    for name in ("nmi_config_parse_lens", "nmi_config_load_lens"):
        assert name in hostapi.EXPORTED_SYMBOLS and hasattr(raw, name), name
    assert lib.nmi_abi_version() == 2  # additive: no bump


def test_undistort_frame_fisheye_rejects_before_touching_a_device(lib):
    fake, fake2, fake3 = C.c_void_p(16), C.c_void_p(32), C.c_void_p(48)   # never dereferenced: every call is rejected first
    K, kp = dbl(fnp.pinhole_K(fnp.raw_K(640, 480), 0.5))
    Kr, krp = dbl(fnp.raw_K(640, 480))
    d, dp = flt(fnp.FAMILIES["strong"])
    E = capi.ERR_INVALID_ARGUMENT
    fn = lib.nmi_undistort_frame_fisheye
    assert fn(None, kp, krp, dp, fake, None, fake2, None) == E          # NULL ctx
    assert fn(fake3, kp, krp, dp, None, None, fake2, None) == E         # NULL raw
    assert fn(fake3, kp, krp, dp, fake, None, None, None) == E          # NULL frame
    assert fn(fake3, None, krp, dp, fake, None, fake2, None) == E       # NULL K
    assert fn(fake3, kp, krp, None, fake, None, fake2, None) == E       # NULL dist
    assert fn(fake3, kp, None, None, fake, None, fake2, None) == E      # NULL dist, K_raw NULL
    assert fn(fake3, kp, krp, dp, fake, None, fake, None) == E          # in place
    assert fn(fake3, kp, krp, dp, fake, None, fake2, fake2) == E        # mask over the frame
    assert fn(fake3, kp, krp, dp, fake, None, fake2, fake) == E         # mask over the raw frame
    assert fn(fake3, kp, krp, dp, fake, fake2, fake2, None) == E        # raw mask over the frame
    for name, k in bad_Ks().items():
        _, bp = dbl(k)
        assert fn(fake3, bp, krp, dp, fake, None, fake2, None) == E, ("K", name)
        assert fn(fake3, kp, bp, dp, fake, None, fake2, None) == E, ("K_raw", name)
        assert fn(fake3, bp, None, dp, fake, None, fake2, None) == E, ("K, K_raw NULL", name)
    for i in range(4):
        for v in (math.nan, math.inf, -math.inf):
            dd = np.array(fnp.FAMILIES["strong"], np.float32)
            dd[i] = v
            _, ddp = flt(dd)
            assert fn(fake3, kp, krp, ddp, fake, None, fake2, None) == E, (i, v)


def test_level_and_stream_fisheye_setters_reject(lib):
    K, kp = dbl(fnp.pinhole_K(fnp.raw_K(640, 480), 0.5))
    Kr, krp = dbl(fnp.raw_K(640, 480))
    d, dp = flt(fnp.FAMILIES["tumvi"])
    E = capi.ERR_INVALID_ARGUMENT
    for fn in (lib.nmi_level_set_distortion_fisheye, lib.nmi_stream_set_distortion_fisheye):
        assert fn(None, kp, krp, dp) == E
        assert fn(None, None, None, None) == E
        for name, k in bad_Ks().items():
            _, bp = dbl(k)
            assert fn(C.c_void_p(16), bp, krp, dp) == E, ("K", name)
            assert fn(C.c_void_p(16), kp, bp, dp) == E, ("K_raw", name)
            assert fn(C.c_void_p(16), bp, None, dp) == E, ("K, K_raw NULL", name)
        assert fn(C.c_void_p(16), None, krp, dp) == E
        dd = np.array(fnp.FAMILIES["tumvi"], np.float32)
        dd[3] = math.nan
        _, ddp = flt(dd)
        assert fn(C.c_void_p(16), kp, krp, ddp) == E


def test_python_wrappers_have_the_fisheye_methods():
    assert callable(getattr(capi.NmiContext, "undistort_frame_fisheye", None))
    assert callable(getattr(capi.NmiLevel, "set_distortion_fisheye", None))
    assert callable(getattr(capi.NmiStream, "set_distortion_fisheye", None))
    assert callable(hostapi.config_parse_lens) and callable(hostapi.config_load_lens)


@pytest.mark.parametrize("scale", fnp.FOCAL_SCALES)
@pytest.mark.parametrize("family", fnp.REGULAR)
def test_twin_source_coordinate_within_rho_of_float64(family, scale):
    """|xs - u_d| + |ys - v_d| <= RHO on every pixel whose source is in reach: the bound the float64 criterion of the GPU tests
    (tests/test_fisheye.py) derives tau from.  (folded is left out: its polynomial cancels and the error reaches 7e-4; the
    others stay under 2.7e-4.)"""
    for W, H in SIZES:
        Kr = fnp.raw_K(W, H)
        K = fnp.pinhole_K(Kr, scale)
        xs, ys = fnp.source_coords((H, W), K, Kr, fnp.FAMILIES[family])
        u, v = fnp.source_coords_f64((H, W), K, Kr, fnp.FAMILIES[family])
        reach = (u > -3) & (u < W + 2) & (v > -3) & (v < H + 2)
        assert reach.sum() > 0.3 * W * H, (W, H, family, scale)
        err = (np.abs(xs - u) + np.abs(ys - v))[reach].max()
        assert err <= RHO, (W, H, family, scale, err)


def test_atan32_is_an_arctangent():
    """The spelled-out arctangent against np.arctan over the radii a pinhole output can have, all three branches."""
    r = np.concatenate([np.linspace(0, 0.5, 20001), np.linspace(0.4, 2.5, 20001), np.linspace(2.4, 40, 20001)]).astype(np.float32)
    t = fnp.atan32(r)
    assert t.dtype == np.float32
    assert np.abs(t.astype(np.float64) - np.arctan(r.astype(np.float64))).max() <= 2.0 ** -22   # 2 ulp of pi / 2
    assert fnp.atan32(np.float32([0]))[0] == 0


def test_folded_family_folds_and_others_do_not():
    """The premise of the families: along the row through the principal point the radius of td grows with the pixel's, for
    every family but folded, whose map turns back inside the frame."""
    W, H = 640, 480
    Kr = fnp.raw_K(W, H)
    for scale in fnp.FOCAL_SCALES:
        K = fnp.pinhole_K(Kr, scale)
        row, c0 = int(round(K[1, 2])), int(math.ceil(K[0, 2]))
        for fam, coeffs in fnp.FAMILIES.items():
            xs, _ = fnp.source_coords((H, W), K, Kr, coeffs)
            monotone = (np.diff(xs[row, c0:].astype(np.float64)) > 0).all() and (np.diff(xs[row, :c0].astype(np.float64)) > 0).all()
            assert monotone == (fam != "folded"), (fam, scale)


def test_focal_scales_leave_the_borders_they_should():
    """Focal scale 0.35 widens the view past the raw frame (an invalid border, not everything); focal scale 1 with the ideal
    lens pulls every source towards the centre: no invalid pixel around the frame centre."""
    for W, H in [(640, 480), (333, 97)]:
        Kr = fnp.raw_K(W, H)
        img = np.zeros((H, W), np.uint8)
        for fam in fnp.REGULAR:
            _, m = fnp.undistort(img, fnp.pinhole_K(Kr, 0.35), Kr, fnp.FAMILIES[fam])
            assert 0 < m.sum() < W * H, (W, H, fam)
        _, m = fnp.undistort(img, Kr, None, fnp.FAMILIES["zero"])
        assert (m[H // 4:3 * H // 4, W // 4:3 * W // 4] == 1).all()


def test_K_raw_none_is_K_in_the_twin():
    W, H = 333, 97
    K = fnp.raw_K(W, H)
    a = fnp.source_coords((H, W), K, None, fnp.FAMILIES["strong"])
    b = fnp.source_coords((H, W), K, K, fnp.FAMILIES["strong"])
    assert (a[0] == b[0]).all() and (a[1] == b[1]).all()


def test_fisheye_image_inverts_the_model():
    """fisheye_image followed by the twin's undistortion gives the pinhole image back where the lens saw it, within one step
    of smooth_frame's quantisation (4: each of the two bilinear resamplings stays inside the local range of the image).  A
    margin of 8 pixels keeps away from the pinhole image's zero border: near the corners a raw pixel spans up to 0.5 /
    cos^2(1.1) = 2.4 pinhole pixels, and the undistortion's taps reach one raw pixel further."""
    from test_warp_edges import smooth_frame
    W, H = 333, 97
    Kr = fnp.raw_K(W, H)
    K = fnp.pinhole_K(Kr, 0.5)
    img = smooth_frame(W, H)
    for fam in fnp.REGULAR:
        raw = fnp.fisheye_image(img, K, Kr, fnp.FAMILIES[fam])
        back, m = fnp.undistort(raw, K, Kr, fnp.FAMILIES[fam])
        inner = np.zeros((H, W), bool)
        inner[8:-8, 8:-8] = True
        inner &= m == 1
        assert inner.sum() > 0.3 * W * H
        assert np.abs(back.astype(int) - img.astype(int))[inner].max() <= 4, fam


KB8 = """%YAML:1.0
Camera.type: "KannalaBrandt8"
Camera.fx: 190.97847715128717
Camera.fy: 190.9733070521226
Camera.cx: 254.93170605935475
Camera.cy: 256.8974428996504
Camera.k1: 0.0034823894022493434
Camera.k2: 0.0007150348452162257
Camera.k3: -0.0020532361418706202
Camera.k4: 0.00020293673591811182
Camera.p1: 0.5
"""


def test_parse_lens_fisheye(tmp_path):
    model, d = hostapi.config_parse_lens(KB8)
    assert model == hostapi.LENS_FISHEYE == 1 and d.dtype == np.float32 and d.shape == (5,)
    assert (d == np.array([0.0034823894022493434, 0.0007150348452162257, -0.0020532361418706202, 0.00020293673591811182, 0], np.float32)).all()
    no_k4 = "\n".join(line for line in KB8.splitlines() if not line.startswith("Camera.k4")) + "\n"
    model, d3 = hostapi.config_parse_lens(no_k4)
    assert model == 1 and d3[3] == 0 and (d3[:3] == d[:3]).all()     # a missing coefficient reads as 0
    p = tmp_path / "kb8.yaml"
    p.write_text(KB8)
    lm, ld = hostapi.config_load_lens(p)
    assert lm == 1 and (ld == d).all()
    with pytest.raises(ValueError):
        hostapi.config_load_lens(tmp_path / "missing.yaml")


def test_parse_lens_pinhole_is_parse_distortion():
    files = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "reference_settings", "*.yaml")))
    assert files
    for f in files:
        model, d = hostapi.config_load_lens(f)
        assert model == hostapi.LENS_RADTAN == 0
        assert (d == hostapi.config_load_distortion(f)).all(), f
    from test_undistort_api import SETTINGS
    five = SETTINGS + "Camera.k3: -0.0123\n"
    for text in (five, five + 'Camera.type: "PinHole"\n'):
        model, d = hostapi.config_parse_lens(text)
        assert model == 0 and (d == hostapi.config_parse_distortion(five)).all() and d[4] == np.float32(-0.0123)


def test_parse_lens_errors(lib):
    raw = b"%YAML:1.0\nthis line has no colon\n"
    model, out = C.c_int32(-1), np.zeros(5, np.float32)
    lens = hostapi._lib().nmi_config_parse_lens
    assert lens(raw, len(raw), C.byref(model), out.ctypes.data_as(C.POINTER(C.c_float))) == -2
    assert lens(None, 0, C.byref(model), out.ctypes.data_as(C.POINTER(C.c_float))) == -1
    assert lens(raw, len(raw), None, out.ctypes.data_as(C.POINTER(C.c_float))) == -1
    assert lens(raw, len(raw), C.byref(model), None) == -1
    with pytest.raises(ValueError):
        hostapi.config_parse_lens('%YAML:1.0\nCamera.type: "Rectified"\n')   # a model this reader does not know
