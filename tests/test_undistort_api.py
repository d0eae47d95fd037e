"""CPU checks of the lens-distortion boundary (include/nmi_hip.h: nmi_undistort_frame, nmi_level_set_distortion,
nmi_stream_set_distortion; include/nmi_host.h: nmi_config_parse_distortion / _load_distortion) and of the numpy twin against the
float64 model.  No device needed: every call below is rejected before anything touches a device."""
import ctypes as C
import glob
import math
import os

import numpy as np
import pytest

from conftest import ROOT
from helpers import undistort_np as unp
from orbslam2_nmi_amd import build as nmi_build
from orbslam2_nmi_amd import capi, hostapi
from orbslam2_nmi_amd import synthetic as sy

UNDISTORT = ("nmi_undistort_frame", "nmi_level_set_distortion", "nmi_stream_set_distortion")
RHO = 2.0 ** -11   # the fp32 source coordinate's error bound of tests/test_warp_edges.py


@pytest.fixture(scope="module")
def lib():
    nmi_build.build()
    return capi.load_library()


def dbl(a):
    a = np.ascontiguousarray(a, np.float64).reshape(-1)
    return a, a.ctypes.data_as(C.POINTER(C.c_double))


def flt(a):
    a = np.ascontiguousarray(a, np.float32).reshape(-1)
    return a, a.ctypes.data_as(C.POINTER(C.c_float))


def test_undistort_symbols_declared_bound_exported(lib):
    from test_capi_symbols import declared_symbols
    raw = C.CDLL(capi.library_path())
    for name in UNDISTORT:
        assert name in declared_symbols(), name
        assert name in capi.EXPORTED_SYMBOLS, name
        assert hasattr(raw, name), f"libnmi_hip.so does not export {name}"
        assert getattr(lib, name).argtypes, f"{name} has no argtypes"
    for name in ("nmi_config_parse_distortion", "nmi_config_load_distortion"):
        assert name in hostapi.EXPORTED_SYMBOLS and hasattr(raw, name), name
    assert lib.nmi_abi_version() == 2  # additive: no bump


def bad_Ks():
    K = sy.intrinsics(640, 480)
    out = {}
    for name, (i, v) in {"skew": (1, 0.5), "row1": (3, 1.0), "row2a": (6, 1e-3), "row2b": (7, 1e-3), "nonunit": (8, 2.0),
                         "fx0": (0, 0.0), "fx<0": (0, -400.0), "fy0": (4, 0.0), "fy<0": (4, -1.0), "fxnan": (0, math.nan),
                         "cxinf": (2, math.inf), "cynan": (5, math.nan), "fxinf": (0, math.inf), "tiny": (0, 1e-300)}.items():
        k = K.copy().reshape(9)
        k[i] = v
        out[name] = k
    return out


def test_undistort_frame_rejects_before_touching_a_device(lib):
    fake = C.c_void_p(16)      # never dereferenced: every call below is rejected first
    fake2 = C.c_void_p(32)
    fake3 = C.c_void_p(48)
    K, kp = dbl(sy.intrinsics(640, 480))
    d, dp = flt(unp.FAMILIES["barrel"])
    E = capi.ERR_INVALID_ARGUMENT
    assert lib.nmi_undistort_frame(None, kp, dp, fake, None, fake2, None) == E          # NULL ctx
    assert lib.nmi_undistort_frame(fake3, kp, dp, None, None, fake2, None) == E         # NULL raw
    assert lib.nmi_undistort_frame(fake3, kp, dp, fake, None, None, None) == E          # NULL frame
    assert lib.nmi_undistort_frame(fake3, None, dp, fake, None, fake2, None) == E       # NULL K
    assert lib.nmi_undistort_frame(fake3, kp, None, fake, None, fake2, None) == E       # NULL dist
    assert lib.nmi_undistort_frame(fake3, kp, dp, fake, None, fake, None) == E          # in place
    assert lib.nmi_undistort_frame(fake3, kp, dp, fake, None, fake2, fake2) == E        # mask over the frame
    assert lib.nmi_undistort_frame(fake3, kp, dp, fake, None, fake2, fake) == E         # mask over the raw frame
    for name, k in bad_Ks().items():
        _, bp = dbl(k)
        assert lib.nmi_undistort_frame(fake3, bp, dp, fake, None, fake2, None) == E, name
    for i in range(5):
        for v in (math.nan, math.inf, -math.inf):
            dd = np.array(unp.FAMILIES["strong_k3"], np.float32)
            dd[i] = v
            _, ddp = flt(dd)
            assert lib.nmi_undistort_frame(fake3, kp, ddp, fake, None, fake2, None) == E, (i, v)


def test_level_and_stream_setters_reject(lib):
    K, kp = dbl(sy.intrinsics(640, 480))
    d, dp = flt(unp.FAMILIES["barrel"])
    E = capi.ERR_INVALID_ARGUMENT
    for fn in (lib.nmi_level_set_distortion, lib.nmi_stream_set_distortion):
        assert fn(None, kp, dp) == E
        assert fn(None, None, None) == E
        for name, k in bad_Ks().items():
            _, bp = dbl(k)
            assert fn(C.c_void_p(16), bp, dp) == E, name
        assert fn(C.c_void_p(16), None, dp) == E
        dd = np.array(unp.FAMILIES["barrel"], np.float32)
        dd[2] = math.nan
        _, ddp = flt(dd)
        assert fn(C.c_void_p(16), kp, ddp) == E


def test_python_wrappers_have_the_methods():
    assert callable(getattr(capi.NmiContext, "undistort_frame", None))
    assert callable(getattr(capi.NmiLevel, "set_distortion", None)) and callable(getattr(capi.NmiStream, "set_distortion", None))


def test_parse_distortion_reference_settings_are_rectified():
    files = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "reference_settings", "*.yaml")))
    assert files
    for f in files:
        d = hostapi.config_load_distortion(f)
        assert d.dtype == np.float32 and d.shape == (5,)
        assert (d == 0).all(), (f, d)
        assert (hostapi.config_parse_distortion(open(f).read()) == d).all()


SETTINGS = """%YAML:1.0
Camera.fx: 458.654
Camera.fy: 457.296
Camera.cx: 367.215
Camera.cy: 248.375
Camera.k1: -0.28340811
Camera.k2: 0.07395907
Camera.p1: 0.00019359
Camera.p2: 1.76187114e-05
"""


def test_parse_distortion_k3_absent_and_all_five(tmp_path):
    d = hostapi.config_parse_distortion(SETTINGS)
    assert (d == np.array([-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05, 0.0], np.float32)).all()
    five = SETTINGS + "Camera.k3: -0.0123\n"
    d5 = hostapi.config_parse_distortion(five)
    assert (d5 == np.array([-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05, -0.0123], np.float32)).all()
    p = tmp_path / "s.yaml"
    p.write_text(five)
    assert (hostapi.config_load_distortion(p) == d5).all()
    with pytest.raises(ValueError):
        hostapi.config_load_distortion(tmp_path / "missing.yaml")


def test_zero_coefficients_are_the_identity_in_the_twin():
    for W, H in [(640, 480), (333, 97), (1, 1)]:
        K = sy.intrinsics(W, H)
        xs, ys = unp.source_coords((H, W), K, np.zeros(5))
        vv, uu = np.mgrid[0:H, 0:W]
        assert (xs == uu).all() and (ys == vv).all()
        img = np.random.default_rng(1).integers(0, 256, (H, W), dtype=np.uint8)
        f, m = unp.undistort(img, K, np.zeros(5))
        assert (f == img).all() and (m == 1).all()


@pytest.mark.parametrize("family", list(unp.FAMILIES))
def test_twin_source_coordinate_within_rho_of_float64(family):
    """|xs - u_d| + |ys - v_d| <= RHO on every pixel whose source is in reach: the bound the float64 criterion of the GPU tests
    (tests/test_undistort.py) derives tau from."""
    for W, H in [(640, 480), (848, 480), (1241, 376), (333, 97)]:
        K = sy.intrinsics(W, H)
        xs, ys = unp.source_coords((H, W), K, unp.FAMILIES[family])
        u, v = unp.source_coords_f64((H, W), K, unp.FAMILIES[family])
        reach = (u > -3) & (u < W + 2) & (v > -3) & (v < H + 2)
        assert reach.sum() > 0.3 * W * H, (W, H, family)
        err = np.abs(xs - u)[reach].max() + np.abs(ys - v)[reach].max()
        assert err <= RHO, (W, H, family, err)


def test_folded_family_folds_and_others_do_not():
    """The premise of the families: the folded one really folds over inside the frame (xs stops growing along a row)."""
    W, H = 640, 480
    K = sy.intrinsics(W, H)
    for fam, coeffs in unp.FAMILIES.items():
        xs, _ = unp.source_coords((H, W), K, coeffs)
        monotone = (np.diff(xs[H // 2].astype(np.float64)) > 0).all()
        if fam in ("barrel", "pincushion", "tangential", "folded"):
            assert monotone == (fam != "folded"), fam
