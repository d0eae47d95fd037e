"""The depth shade (include/nmi_hip.h, "Depth maps"), CPU tier: the numpy twin (tests/helpers/depth_np.py) against a float64 model
of the same formula over all 2^24 depths, its monotonicity, known answers, and the new entry points' symbols and argument errors
(no device is needed for those: a bad shade is refused before the context is looked at).

Twin against model: the fp32 chain is five correctly rounded operations on positive values (u, the product u (far - near), the
sum, near far, the quotient) plus the product with the scale and the + 0.5: a relative error below 6 * 2^-24 on z, hence below
65535 * 6 * 2^-24 = 0.03 raw units on z * scale wherever v is not clamped -- only the final truncation can differ, by one unit.
"""
import ctypes as C

import numpy as np
import pytest

from helpers import depth_np as dn
from orbslam2_nmi_amd import capi

f32 = np.float32
PROJECTIONS = [(0.1, 100.0, 1000.0), (0.05, 1000.0, 1000.0), (0.3, 10.0, 5000.0), (1.0, 65.0, 1000.0)]   # near, far, scale
ALL_DEPTHS = np.arange(1 << 24, dtype=np.int64)


@pytest.fixture(scope="module", params=PROJECTIONS, ids=[f"{n}-{f}-x{s:g}" for n, f, s in PROJECTIONS])
def both(request):
    """(shade, v32 over all depths, v64 over all depths): computed once per projection and shared."""
    near, far, scale = request.param
    sh = dn.make(near, far, scale, 1000, 60000)
    v32 = dn.raw_depth(ALL_DEPTHS, sh, f32)
    v64 = dn.raw_depth(ALL_DEPTHS, sh, np.float64)
    v32.setflags(write=False), v64.setflags(write=False)
    return sh, v32, v64


def test_twin_meets_float64_model_on_all_depths(both):
    sh, v32, v64 = both
    worst = int(np.abs(v32 - v64).max())
    print(f"{sh}: largest |v32 - v64| = {worst}, {int((v32 != v64).sum())} of 2^24 depths differ")
    assert worst <= 1


def test_raw_depth_is_monotone(both):
    _, v32, v64 = both
    assert (np.diff(v32) >= 0).all() and (np.diff(v64) >= 0).all()


def test_known_answers_at_the_planes(both):
    sh, v32, _ = both
    near, far, scale = sh["near_plane"], sh["far_plane"], sh["scale"]
    want_near = min(max(int(np.floor(near * scale + 0.5)), 1), 65535)
    want_far = min(max(int(np.floor(far * scale + 0.5)), 1), 65535)
    assert abs(int(v32[0]) - want_near) <= 1, (int(v32[0]), want_near)
    assert abs(int(v32[-1]) - want_far) <= 1, (int(v32[-1]), want_far)
    assert v32.min() >= 1 and v32.max() <= 65535


def test_clamps():
    # 0.3 m .. 10 m at 7000 units per metre: 2100 .. 70000, the far part of the range passes 65535; at 1e-4 units per metre
    # everything rounds to 0 and is lifted to 1
    hi = dn.raw_depth(ALL_DEPTHS[-4096:], dn.make(0.3, 10.0, 7000.0, 1, 2), f32)
    assert (hi == 65535).all()
    lo = dn.raw_depth(ALL_DEPTHS[::4097], dn.make(0.3, 10.0, 1e-4, 1, 2), f32)
    assert (lo == 1).all()
    v, g = dn.shade(np.array([0, 5, -1, dn.D_MAX]), dn.make(0.3, 10.0, 7000.0, 2100, 65535), empty=-1)
    assert v[2] == 0 and g[2] == 255 and v[0] == 2100 and g[0] == 0 and v[3] == 65535 and g[3] == 255


@pytest.mark.parametrize("lo,hi", [(0, 65535), (1000, 60000), (4999, 5001), (5000, 5001), (0, 1)])
def test_window_ends(lo, hi):
    v = np.array([0, 1, lo, lo + 1, (lo + hi) // 2, hi - 1, hi, 65535])
    g = dn.window_rule(v, lo, hi).astype(np.int64)
    assert g[2] == 0 and g[6] == 255 and g[0] == 0 and g[7] == 255
    assert g[3] == (255 + ((hi - lo) >> 1)) // (hi - lo)
    assert g[5] == ((hi - 1 - lo) * 255 + ((hi - lo) >> 1)) // (hi - lo) or hi - 1 == lo
    assert (np.diff(dn.window_rule(np.arange(65536), lo, hi).astype(np.int64)) >= 0).all()
    # the intake's rule (tests/helpers/tone_np.py), which the camera side applies to its depth frame: one mapping on both sides
    from helpers import tone_np as tn
    assert (dn.window_rule(np.arange(65536), lo, hi) == tn.window_rule(np.arange(65536), lo, hi)).all()


# ----------------------------------------------------------------------------------------------------- symbols, argument errors
NEW = ("nmi_render_points_depth", "nmi_render_mesh_depth", "nmi_depth_shade_apply", "nmi_level_create_depth",
       "nmi_level_create_depth_block", "nmi_level_set_depth_shade")


def bad_shades():
    ok = dict(near_plane=0.5, far_plane=50.0, scale=1000.0, lo=500, hi=50000)
    out = []
    for k in ("near_plane", "far_plane", "scale"):
        out += [dict(ok, **{k: x}) for x in (float("nan"), float("inf"), -float("inf"))]
    out += [dict(ok, near_plane=0.0), dict(ok, near_plane=-1.0), dict(ok, far_plane=0.5), dict(ok, far_plane=0.25), dict(ok, scale=0.0),
            dict(ok, scale=-1.0), dict(ok, lo=-1), dict(ok, lo=50000), dict(ok, lo=50001), dict(ok, hi=65536), dict(ok, lo=0, hi=0)]
    shades = [capi.NmiDepthShade(**d) for d in out]
    for i in range(3):
        s = capi.NmiDepthShade(**ok)
        s.reserved[i] = 1
        shades.append(s)
    return capi.NmiDepthShade(**ok), shades


def test_new_symbols_and_abi_version():
    lib = capi.load_library()
    raw = C.CDLL(capi.library_path())
    for name in NEW:
        assert name in capi.EXPORTED_SYMBOLS and hasattr(raw, name), name
    assert lib.nmi_abi_version() == 2
    assert C.sizeof(capi.NmiDepthShade) == 32


def test_argument_errors_without_a_device():
    lib = capi.load_library()
    E = capi.ERR_INVALID_ARGUMENT
    good, bad = bad_shades()
    fake = C.c_void_p(4096)    # never read: every call below is refused on its arguments
    mvp = (C.c_float * 16)(*np.eye(4, dtype=f32).reshape(16))
    lv = C.c_void_p()
    for sh in [None] + bad:
        ref = C.byref(sh) if sh is not None else None
        assert lib.nmi_render_points_depth(fake, fake, None, 1, mvp, 1, 1.0, ref, fake, None, None) == E
        assert lib.nmi_render_mesh_depth(fake, fake, 1, mvp, 1, ref, fake, None, None) == E
        assert lib.nmi_depth_shade_apply(fake, ref, fake, 1, fake, fake) == E
        assert lib.nmi_level_create_depth(fake, capi.MAP_POINTS, fake, 1, fake, 1, 1, 1.0, ref, C.byref(lv)) == E and not lv.value
        assert lib.nmi_level_create_depth_block(fake, capi.MAP_MESH, fake, 1, fake, 1, 0, 1, 1, 0, 1, 1.0, ref, C.byref(lv)) == E and not lv.value
        if sh is not None:
            assert lib.nmi_level_set_depth_shade(fake, ref) == E     # (a bad shade is refused without reading the level)
    g = C.byref(good)
    # a good shade: the renderers' usual cases, all before any device call
    assert lib.nmi_render_points_depth(None, fake, None, 1, mvp, 1, 1.0, g, fake, None, None) == E
    assert lib.nmi_render_mesh_depth(None, fake, 1, mvp, 1, g, fake, None, None) == E
    assert lib.nmi_depth_shade_apply(None, g, fake, 1, fake, fake) == E
    assert lib.nmi_level_set_depth_shade(None, g) == E and lib.nmi_level_set_depth_shade(None, None) == E
    for kind in (-1, 2):
        assert lib.nmi_level_create_depth(fake, kind, fake, 1, fake, 1, 1, 1.0, g, C.byref(lv)) == E and not lv.value
    for S, Wn in ((0, 1), (1, 0), (-1, 1)):
        assert lib.nmi_level_create_depth(fake, capi.MAP_MESH, fake, 1, fake, S, Wn, 1.0, g, C.byref(lv)) == E and not lv.value
    assert lib.nmi_level_create_depth(None, capi.MAP_MESH, fake, 1, fake, 1, 1, 1.0, g, C.byref(lv)) == E and not lv.value


def test_window_quotient_without_integer_division():
    """The kernel takes the window's quotient as (uint32)((float)n * (1 / (float)span)) mended by the remainder's sign
    (csrc/nmi_depth_device.h).  The same fp32 arithmetic in numpy, for EVERY span and, per span, the ends of the window, the values
    around every eighth of it and 48 random ones: equal to the integer rule."""
    rng = np.random.default_rng(11)
    span = np.arange(1, 65536, dtype=np.int64)[:, None]
    eighths = (span * np.arange(9)[None, :]) // 8
    c = np.concatenate([eighths, eighths + 1, eighths - 1, rng.integers(0, 65536, (65535, 48)) % (span + 1)], 1)
    c = np.clip(c, 0, span)
    n = c * 255 + (span >> 1)
    assert n.max() < 1 << 24
    inv = f32(1.0) / span.astype(f32)
    q = (n.astype(f32) * inv).astype(np.int64)
    r = n - q * span
    q = q + (r >= span) - (r < 0)
    assert (q == n // span).all() and q.max() == 255 and q.min() == 0
