"""CPU checks of the colour-frame boundary: Camera.RGB from the settings files (include/nmi_host.h:
nmi_config_parse_color_order / _load_color_order), the declarations and bindings of nmi_gray_frame, nmi_level_set_frame_format
and nmi_stream_set_frame_format, the rejections that need no device, and the numpy twin of the rule (tests/helpers/color_np.py)."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

from conftest import ROOT
from helpers import color_np as cnp
from orbslam2_nmi_amd import build as nmi_build
from orbslam2_nmi_amd import capi, hostapi

COLOR = ("nmi_gray_frame", "nmi_level_set_frame_format", "nmi_stream_set_frame_format")


@pytest.fixture(scope="module")
def lib():
    nmi_build.build()
    return capi.load_library()


def test_color_symbols_declared_bound_exported(lib):
    from test_capi_symbols import declared_symbols
    raw = C.CDLL(capi.library_path())
    for name in COLOR:
        assert name in declared_symbols(), name
        assert name in capi.EXPORTED_SYMBOLS, name
        assert hasattr(raw, name), f"libnmi_hip.so does not export {name}"
        assert getattr(lib, name).argtypes, f"{name} has no argtypes"
    for name in ("nmi_config_parse_color_order", "nmi_config_load_color_order"):
        assert name in hostapi.EXPORTED_SYMBOLS and hasattr(raw, name), name
    assert lib.nmi_abi_version() == 2  # additive: no bump
    assert (capi.FRAME_GRAY, capi.FRAME_BGR, capi.FRAME_RGB, capi.FRAME_BGRA, capi.FRAME_RGBA) == (0, 1, 2, 3, 4)
    assert all(callable(getattr(c, "set_frame_format", None)) for c in (capi.NmiLevel, capi.NmiStream))
    assert callable(getattr(capi.NmiContext, "gray_frame", None))


def test_null_handles_are_rejected_before_any_device(lib):
    assert lib.nmi_gray_frame(None, None, 2, 0, None) == capi.ERR_INVALID_ARGUMENT
    assert lib.nmi_level_set_frame_format(None, 2, 0) == capi.ERR_INVALID_ARGUMENT
    assert lib.nmi_stream_set_frame_format(None, 2, 0) == capi.ERR_INVALID_ARGUMENT


def settings_files():
    files = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "reference_settings", "*.yaml")))
    assert len(files) == 7
    return files + [os.path.join(ROOT, "tests", "golden", "settings_example.yaml")]


@pytest.mark.parametrize("path", settings_files(), ids=os.path.basename)
def test_reference_settings_are_rgb(path):
    assert hostapi.config_load_color_order(path) == 1
    with open(path) as f:
        assert hostapi.config_parse_color_order(f.read()) == 1


BASE = """%YAML:1.0
Camera.fx: 458.654
Camera.fy: 457.296
Camera.cx: 367.215
Camera.cy: 248.375
"""


def test_explicit_zero_missing_key_and_errors(tmp_path):
    assert hostapi.config_parse_color_order(BASE + "Camera.RGB: 0\n") == 0
    assert hostapi.config_parse_color_order(BASE + "Camera.RGB: 1\n") == 1
    assert hostapi.config_parse_color_order(BASE) == 0                     # missing key: BGR, as cv::FileNode gives it
    p = tmp_path / "s.yaml"
    p.write_text(BASE + "Camera.RGB: 0\n")
    assert hostapi.config_load_color_order(p) == 0
    # the distortion pair's codes: -2 syntax, -5 unreadable, -1 NULL
    bad = b"%YAML:1.0\nCamera.RGB 1\n"   # a top-level line without a colon
    out = C.c_int32(7)
    lib = hostapi._lib()
    assert lib.nmi_config_parse_distortion(bad, len(bad), (C.c_float * 5)()) == -2
    assert lib.nmi_config_parse_color_order(bad, len(bad), C.byref(out)) == -2
    assert lib.nmi_config_load_color_order(str(tmp_path / "missing.yaml").encode(), C.byref(out)) == -5
    assert lib.nmi_config_load_distortion(str(tmp_path / "missing.yaml").encode(), (C.c_float * 5)()) == -5
    assert lib.nmi_config_parse_color_order(None, 0, C.byref(out)) == -1
    assert lib.nmi_config_parse_color_order(b"a: 1\n", 5, None) == -1
    with pytest.raises(ValueError):
        hostapi.config_load_color_order(tmp_path / "missing.yaml")


def test_twin_maps_equal_channels_to_that_grey():
    g = np.arange(256)
    assert (cnp.gray_of(g, g, g) == g).all()
    assert 4899 + 9617 + 1868 == 1 << 14


def test_twin_layouts_round_trip():
    rng = np.random.default_rng(3)
    h, w = 5, 7
    rgb = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    want = cnp.gray_of(rgb[..., 0], rgb[..., 1], rgb[..., 2])
    for fmt in cnp.COLOR_FORMATS:
        for pitch, off in [(0, 0), (w * cnp.BPP[fmt] + 5, 3)]:
            buf = cnp.pack(rgb, fmt, pitch, off, seed=fmt)
            assert buf.size == off + cnp.span(fmt, w, h, pitch)
            assert (cnp.to_gray(buf, fmt, w, h, pitch, off) == want).all()
    g = rgb[..., 0]
    assert (cnp.to_gray(cnp.pack(g, cnp.GRAY, w + 1, 1), cnp.GRAY, w, h, w + 1, 1) == g).all()
    # BGR is RGB with R and B swapped
    bgr = cnp.pack(rgb, cnp.BGR)
    assert (cnp.to_gray(bgr, cnp.RGB, w, h) == cnp.gray_of(rgb[..., 2], rgb[..., 1], rgb[..., 0])).all()
