"""The form matrix of the point renderer's resolve pass (csrc/nmi_producers.hip, launch_resolve): every instantiation the launcher
can choose runs once, at the smallest shape that reaches it.

  fast form      nmi_zbuf_resolve_fast_kernel<SIZE, COVER, Shade...>: 64x48 (width % 4 == 0), point sizes 1 .. 5, coverage off / on,
                 the map's colour / its depth with an 8-byte-aligned depth16
  any-size form  nmi_zbuf_resolve_kernel<COVER, Shade...>, reached three ways: 62x47 (width % 4 != 0), point size 6 at 64x48, and a
                 depth16 stack offset by one element (2-byte aligned; depth renders only)

`==` on every byte against the committed twins: oracle/render_oracle_np.py (colour, coverage = the twin's own key test) and
tests/helpers/depth_np.py (grey, raw depths).  A render with coverage is byte-identical to the one without.
S = 2 views of 300 points; the references are computed once per (frame, point size) and shared.
"""
import functools

import numpy as np
import pytest

from helpers import depth_np as dn
from helpers import render_cases as rc
from oracle import render_oracle_np as ro

try:
    import torch
except ImportError:  # collection without torch
    torch = None

f32 = np.float32
SHADE = dn.make(rc.ZN, rc.ZF, 1000.0, 6000, 28000)   # millimetres, a window inside the range: both of its ends are reached
N_POINTS = 300
# (width, height, point size, depth16 offset in elements)
FAST = [(64, 48, size, 0) for size in (1, 2, 3, 4, 5)]
ANY = [(62, 47, 3, 0), (64, 48, 6, 0)]
ANY_DEPTH_ONLY = [(64, 48, 3, 1)]
CASES = [(form, cover, kind) for form in FAST + ANY for cover in (False, True) for kind in ("colour", "depth")]
CASES += [(form, cover, "depth") for form in ANY_DEPTH_ONLY for cover in (False, True)]


def case_id(c):
    (W, H, size, off), cover, kind = c
    return f"{W}x{H}-size{size}-{'cover' if cover else 'plain'}-{kind}" + ("-depth16+1" if off else "")


@functools.lru_cache(maxsize=None)
def scene(W, H):
    """300 points spread over (and a little beyond) the window of the axis camera, at all depths; two views of them."""
    rng = np.random.default_rng(W * 1000 + H)
    cams = rc.cameras(W, H)
    mvps = np.stack([cams["axis"], cams["rolled"]])
    xw, yw = rng.uniform(-2.0, W + 2.0, N_POINTS), rng.uniform(-2.0, H + 2.0, N_POINTS)
    xyz = rc.unproject(cams["axis"], W, H, xw, yw, rng.uniform(0.05, 0.98, N_POINTS)).astype(f32)
    return xyz, rng.uniform(0.0, 1.0, N_POINTS).astype(f32), mvps


@functools.lru_cache(maxsize=None)
def reference(W, H, size):
    """-> (colour [S,H,W], coverage, depth grey, depth16) of the scene, from the twins."""
    xyz, red, mvps = scene(W, H)
    colour = ro.render_stack(xyz, red, mvps, W, H, size)
    cover = np.stack([ro.coverage(xyz, red, m, W, H, size) for m in mvps])
    grey, v, dcover = dn.points_stack(xyz, red, mvps, W, H, size, SHADE)
    assert (dcover == cover).all() and 0 < cover.sum() < cover.size and len(np.unique(grey)) > 16
    return colour, cover, grey, v


@pytest.fixture(scope="module")
def contexts():
    if torch is None or not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    import orbslam2_nmi_amd as m
    m.load_library()
    open_ = {}

    def get(W, H):
        if (W, H) not in open_:
            open_[(W, H)] = m.NmiContext(W, H)
        return open_[(W, H)]

    yield get
    for ctx in open_.values():
        ctx.close()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_gpu_resolve_form(contexts, case):
    from orbslam2_nmi_amd import capi
    (W, H, size, off), cover, kind = case
    xyz, red, mvps = scene(W, H)
    want_colour, want_cover, want_grey, want_v = reference(W, H, size)
    S = len(mvps)
    ctx = contexts(W, H)
    dx, dr = dev(xyz), dev(red)
    mask = None
    if kind == "colour":
        plain = ctx.render_points(dx, dr, mvps, float(size))
        out = plain
        if cover:
            out, mask = ctx.render_points_masked(dx, dr, mvps, float(size))
        assert (out.cpu().numpy() == want_colour).all()
    else:
        buf = torch.zeros(S * H * W + off, dtype=torch.int16, device="cuda")
        v = buf[off:].view(S, H, W)
        assert v.data_ptr() % 8 == (2 if off else 0)
        shade = capi.NmiDepthShade(**SHADE)
        plain, _, _ = ctx.render_points_depth(dx, dr, mvps, float(size), shade)
        out, mask, _ = ctx.render_points_depth(dx, dr, mvps, float(size), shade, out_masks=True if cover else None, depth16=v)
        assert (mask is not None) == cover
        assert (out.cpu().numpy() == want_grey).all()
        assert (v.cpu().numpy().view(np.uint16) == want_v).all()
        if off:
            assert int(buf[0]) == 0   # nothing before the stack's first element
    assert torch.equal(out, plain)   # with coverage, with depth16: the same render bytes
    if cover:
        assert (mask.cpu().numpy() == want_cover).all()
