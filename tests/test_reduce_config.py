"""CPU checks of the full-size-frame boundary: nmi_config_reduce (include/nmi_host.h), the declarations and bindings of
nmi_reduce_frame, nmi_level_set_frame_reduction and nmi_stream_set_frame_reduction, and the rejections that need no device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from orbslam2_nmi_amd import build as nmi_build
from orbslam2_nmi_amd import capi, hostapi

REDUCE = ("nmi_reduce_frame", "nmi_level_set_frame_reduction", "nmi_stream_set_frame_reduction")
ETH_SMALL = os.path.join(ROOT, "tests", "golden", "reference_settings", "ETH_small.yaml")


@pytest.fixture(scope="module")
def lib():
    nmi_build.build()
    return capi.load_library()


def test_reduce_symbols_declared_bound_exported(lib):
    from test_capi_symbols import declared_symbols
    raw = C.CDLL(capi.library_path())
    for name in REDUCE:
        assert name in declared_symbols(), name
        assert name in capi.EXPORTED_SYMBOLS, name
        assert hasattr(raw, name), f"libnmi_hip.so does not export {name}"
        assert getattr(lib, name).argtypes, f"{name} has no argtypes"
    assert "nmi_config_reduce" in hostapi.EXPORTED_SYMBOLS and hasattr(raw, "nmi_config_reduce")
    assert lib.nmi_abi_version() == 2  # additive: no bump
    assert all(callable(getattr(c, "set_frame_reduction", None)) for c in (capi.NmiLevel, capi.NmiStream))
    assert callable(getattr(capi.NmiContext, "reduce_frame", None))
    assert callable(hostapi.config_reduce)


def test_null_handles_are_rejected_before_any_device(lib):
    assert lib.nmi_reduce_frame(None, None, 2, 0, 2, None, None, None) == capi.ERR_INVALID_ARGUMENT
    assert lib.nmi_level_set_frame_reduction(None, 2, 2, 0) == capi.ERR_INVALID_ARGUMENT
    assert lib.nmi_stream_set_frame_reduction(None, 2, 2, 0) == capi.ERR_INVALID_ARGUMENT


def full_size_text(f):
    """ETH_small.yaml (960x540) rewritten as the settings of the same camera at f times the size: the file a 1920x1080 (f = 2)
    camera would come with.  Returns (text, the search-size Config the file itself gives)."""
    with open(ETH_SMALL) as fh:
        text = fh.read()
    small = hostapi.config_parse(text)

    def put(key, value):
        nonlocal text
        text, n = re.subn(rf"^{re.escape(key)}:.*$", f"{key}: {value!r}", text, flags=re.M)
        assert n == 1, key

    put("Camera.fx", small.fx * f)
    put("Camera.fy", small.fy * f)
    put("Camera.cx", f * (small.cx + 0.5) - 0.5)
    put("Camera.cy", f * (small.cy + 0.5) - 0.5)
    put("Camera.Width", small.width * f)
    put("Camera.Height", small.height * f)
    put("NMI.Render.PointSize", float(small.render_point_size) * f)
    return text, small


@pytest.mark.parametrize("f", [1, 2, 3, 4])
def test_config_reduce_gives_the_search_size_settings(f):
    text, small = full_size_text(f)
    full = hostapi.config_parse(text)
    assert (full.width, full.height) == (960 * f, 540 * f)
    red = hostapi.config_reduce(full, f)
    assert (red.width, red.height) == (960, 540) == (small.width, small.height)
    # the stated values, computed here in double precision from the full-size ones
    assert red.fx == full.fx / f and red.fy == full.fy / f
    assert red.cx == (full.cx + 0.5) / f - 0.5 and red.cy == (full.cy + 0.5) / f - 0.5
    assert np.float32(red.render_point_size) == np.float32(full.render_point_size) / np.float32(f)
    # ... which are the file's own, to a few double-precision roundings of values of a few hundred (the text holds the products)
    for a, b in ((red.fx, small.fx), (red.fy, small.fy), (red.cx, small.cx), (red.cy, small.cy)):
        assert abs(a - b) <= 4 * np.spacing(1024.0), (a, b)
    assert abs(red.render_point_size - small.render_point_size) <= 4 * np.spacing(np.float32(8.0))
    # everything else unchanged; the input is not modified by the Python wrapper
    assert (full.width, full.height) == (960 * f, 540 * f)
    for name in ("nmi_threshold", "init_offset", "has_init1", "has_init2", "render_near", "render_far", "render_object", "render_texture",
                 "render_cloud", "render_offset"):
        assert getattr(red, name) == getattr(full, name), name
    assert list(red.init1) == list(full.init1) and list(red.init2) == list(full.init2)
    assert bytes(red.initial) == bytes(full.initial)
    if f == 1:
        assert bytes(red) == bytes(full)


def test_width_and_height_divide_as_integers():
    text, _ = full_size_text(1)
    cfg = hostapi.config_parse(text)
    cfg.width, cfg.height = 1241, 376
    assert [(c.width, c.height) for c in (hostapi.config_reduce(cfg, f) for f in (2, 3, 4))] == [(620, 188), (413, 125), (310, 94)]


@pytest.mark.parametrize("f", [2, 3, 4])
def test_pixel_mapping_round_trips(f):
    """Output pixel i is centred on source coordinate f i + (f - 1) / 2: a ray through a source pixel centre under the full-size K
    meets the reduced image at the output coordinate of that centre, and back."""
    text, _ = full_size_text(f)
    full = hostapi.config_parse(text)
    red = hostapi.config_reduce(full, f)
    i = np.arange(0, 960, 37, dtype=np.float64)
    for (c_full, f_full, c_red, f_red) in ((full.cx, full.fx, red.cx, red.fx), (full.cy, full.fy, red.cy, red.fy)):
        centre = f * i + (f - 1) / 2              # the centre of output pixel i's block, in source pixels
        ray = (centre - c_full) / f_full
        assert np.allclose(ray * f_red + c_red, i, rtol=0, atol=1e-9)
        back = ((i - c_red) / f_red) * f_full + c_full
        assert np.allclose(back, centre, rtol=0, atol=1e-9)


def test_config_reduce_errors():
    lib = hostapi._lib()
    text, _ = full_size_text(2)
    cfg = hostapi.config_parse(text)
    before = bytes(cfg)
    assert lib.nmi_config_reduce(None, 2) < 0
    for bad in (0, -1, 5, 100):
        assert lib.nmi_config_reduce(C.byref(cfg), bad) < 0, bad
        assert bytes(cfg) == before
        with pytest.raises(ValueError):
            hostapi.config_reduce(cfg, bad)
    assert lib.nmi_config_reduce(C.byref(cfg), 2) == 0
    assert (cfg.width, cfg.height) == (960, 540)
