"""Coverage forms of the renderers (nmi_render_points_masked, nmi_render_mesh_masked) and the whole covered chain on the
device: renders byte-identical to the unmasked calls, masks equal to a black-input render != 255 and to the numpy twins."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import covered_np as cnp
from oracle import mesh_oracle_np as mo
from orbslam2_nmi_amd import capi, synthetic as sy
import orbslam2_nmi_amd as nmi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _device():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    capi.load_library()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def cloud(n, seed, spread=(6, 4, 6), centre=(0, 0, 9)):
    rng = np.random.default_rng(seed)
    xyz = (rng.uniform(-1, 1, (n, 3)) * spread + centre).astype(np.float32)
    red = rng.uniform(0, 1, n).astype(np.float32)
    return xyz, red


def views(w, h, S, seed, size=1.0):
    K = sy.intrinsics(w, h)
    rp = capi.RenderParams(fx=K[0, 0], fy=K[1, 1], cx=K[0, 2], cy=K[1, 2], near_plane=0.5, far_plane=40.0, point_size=size)
    rng = np.random.default_rng(seed)
    return np.stack([capi.render_mvp(rp, (0, 0, 0), (0, 0, 1), (0, -1, 0), tuple(rng.uniform(-0.5, 0.5, 3))) for _ in range(S)])


# ---- 7. points ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [1.0, 2.0, 3.0, 4.0, 5.0, 7.0])
@pytest.mark.parametrize("shape", [(640, 480), (162, 121)], ids=["640x480", "162x121"])
def test_points_masked_equals_render_and_black_render(size, shape):
    w, h = shape
    xyz, red = cloud(4000, 3)
    mvps = views(w, h, 5, 1, size)
    with capi.NmiContext(w, h) as ctx:
        dx, dr = dev(xyz), dev(red)
        plain = ctx.render_points(dx, dr, mvps, size).cpu().numpy()
        img, masks = ctx.render_points_masked(dx, dr, mvps, size)
        dark = ctx.render_points(dx, torch.zeros_like(dr), mvps, size).cpu().numpy()
    img, masks = img.cpu().numpy(), masks.cpu().numpy()
    assert (img == plain).all()
    assert set(np.unique(dark)) <= {0, 255}
    assert (masks == (dark == 0)).all() and set(np.unique(masks)) <= {0, 1}
    assert 0.01 < masks.mean() < 0.99


@pytest.mark.parametrize("size", [1.0, 2.0, 3.0, 5.0])
def test_points_masks_equal_twin(size):
    w, h = 66, 50  # width not a multiple of 4: the general resolve form
    xyz, red = cloud(300, 7)
    mvps = views(w, h, 3, 2, size)
    with capi.NmiContext(w, h) as ctx:
        _, masks = ctx.render_points_masked(dev(xyz), dev(red), mvps, size)
    want = cnp.coverage_twin_points(xyz, mvps, w, h, size)
    assert (masks.cpu().numpy() == want).all()


def test_points_no_points_covers_nothing():
    w, h = 64, 48
    mvps = views(w, h, 2, 3)
    empty = torch.zeros((0, 3), dtype=torch.float32, device="cuda")
    with capi.NmiContext(w, h) as ctx:
        img, masks = ctx.render_points_masked(empty, torch.zeros(0, dtype=torch.float32, device="cuda"), mvps, 2.0)
    assert (img.cpu().numpy() == 255).all() and (masks.cpu().numpy() == 0).all()


def test_points_bool_masks_out():
    w, h = 64, 48
    xyz, red = cloud(200, 9)
    mvps = views(w, h, 2, 4)
    with capi.NmiContext(w, h) as ctx:
        _, m8 = ctx.render_points_masked(dev(xyz), dev(red), mvps, 2.0)
        _, mb = ctx.render_points_masked(dev(xyz), dev(red), mvps, 2.0,
                                         out_masks=torch.empty((2, h, w), dtype=torch.bool, device="cuda"))
    assert (mb.cpu().numpy() == (m8.cpu().numpy() != 0)).all()


# ---- 7. mesh --------------------------------------------------------------------------------------------------------------
def small_mesh(w, h):
    """Quads over part of the view at depth 10, both windings, plus a triangle crossing the near plane."""
    K = sy.intrinsics(w, h)
    rp = capi.RenderParams(fx=K[0, 0], fy=K[1, 1], cx=K[0, 2], cy=K[1, 2], near_plane=1.0, far_plane=30.0, point_size=1.0)
    us, vs = np.linspace(0.2 * w, 0.7 * w, 7), np.linspace(0.3 * h, 0.9 * h, 5)
    uu, vv = np.meshgrid(us, vs)
    z = np.full_like(uu, 10.0)
    P = np.stack([(uu - rp.cx) / rp.fx * z, (vv - rp.cy) / rp.fy * z, z], -1).astype(np.float32)
    T = np.stack([uu / w, vv / h], -1).astype(np.float32)
    p00, p10, p01, p11 = P[:-1, :-1], P[:-1, 1:], P[1:, :-1], P[1:, 1:]
    t00, t10, t01, t11 = T[:-1, :-1], T[:-1, 1:], T[1:, :-1], T[1:, 1:]
    xyz = np.stack([p00, p10, p11, p00, p11, p01], 2).reshape(-1, 3)
    uv = np.stack([t00, t10, t11, t00, t11, t01], 2).reshape(-1, 2)
    near = np.array([[-3, 2, -2.0], [3, 2, 20.0], [-3, 2, 20.0]], np.float32)  # crosses the near plane
    xyz = np.concatenate([xyz, near])
    uv = np.concatenate([uv, np.array([[0, 0], [1, 0], [0, 1]], np.float32)])
    x3, u3 = xyz.reshape(-1, 3, 3), uv.reshape(-1, 3, 2)
    xyz = np.concatenate([x3, x3[:, ::-1]]).reshape(-1, 3).copy()
    uv = np.concatenate([u3, u3[:, ::-1]]).reshape(-1, 2).copy()
    mvps = np.stack([capi.render_mvp(rp, (0, 0, 0), (0, 0, 1), (0, -1, 0), t) for t in ((0, 0, 0), (0.4, -0.3, 1.0), (-0.8, 0.2, -2.0))])
    return xyz, uv, mvps


def test_mesh_masks_equal_twin_and_black_render():
    w, h = 96, 72
    xyz, uv, mvps = small_mesh(w, h)
    rgb = (np.random.default_rng(1).integers(1, 255, (32, 32, 3))).astype(np.uint8)
    with capi.NmiContext(w, h) as ctx, nmi.NmiTexture(ctx, rgb) as tex, nmi.NmiTexture(ctx, np.zeros_like(rgb)) as tb:
        dx, du = dev(xyz), dev(uv)
        plain = ctx.render_mesh(dx, du, tex, mvps).cpu().numpy()
        img, masks = ctx.render_mesh_masked(dx, du, tex, mvps)
        dark = ctx.render_mesh(dx, du, tb, mvps).cpu().numpy()
    img, masks = img.cpu().numpy(), masks.cpu().numpy()
    assert (img == plain).all()
    assert (masks == (dark == 0)).all()
    want = cnp.coverage_twin_mesh(xyz, uv, mvps, w, h)
    assert (masks == want).all(), f"{(masks != want).sum()} pixels differ"
    assert 0.05 < masks.mean() < 0.95


def test_mesh_small_triangles_memory_path():
    """A dense mesh of pixel-sized triangles: pixels won through the memory buffer are covered too."""
    w, h = 160, 120
    K = sy.intrinsics(w, h)
    rp = capi.RenderParams(fx=K[0, 0], fy=K[1, 1], cx=K[0, 2], cy=K[1, 2], near_plane=1.0, far_plane=30.0, point_size=1.0)
    us, vs = np.linspace(0.1 * w, 0.6 * w, 121), np.linspace(0.2 * h, 0.8 * h, 91)
    uu, vv = np.meshgrid(us, vs)
    z = 10.0 + 0.5 * np.sin(uu * 0.1)
    P = np.stack([(uu - rp.cx) / rp.fx * z, (vv - rp.cy) / rp.fy * z, z], -1).astype(np.float32)
    T = np.stack([uu / w, vv / h], -1).astype(np.float32)
    p00, p10, p01, p11 = P[:-1, :-1], P[:-1, 1:], P[1:, :-1], P[1:, 1:]
    t00, t10, t01, t11 = T[:-1, :-1], T[:-1, 1:], T[1:, :-1], T[1:, 1:]
    xyz = np.concatenate([np.stack([p00, p10, p11, p00, p11, p01], 2).reshape(-1, 3), np.stack([p00, p11, p10, p00, p01, p11], 2).reshape(-1, 3)])
    uv = np.concatenate([np.stack([t00, t10, t11, t00, t11, t01], 2).reshape(-1, 2), np.stack([t00, t11, t10, t00, t01, t11], 2).reshape(-1, 2)])
    mvps = np.stack([capi.render_mvp(rp, (0, 0, 0), (0, 0, 1), (0, -1, 0), t) for t in ((0, 0, 0), (0.2, 0.1, 0.5))])
    rgb = np.full((16, 16, 3), 90, np.uint8)
    with capi.NmiContext(w, h) as ctx, nmi.NmiTexture(ctx, rgb) as tex, nmi.NmiTexture(ctx, np.zeros_like(rgb)) as tb:
        dx, du = dev(np.ascontiguousarray(xyz)), dev(np.ascontiguousarray(uv))
        plain = ctx.render_mesh(dx, du, tex, mvps).cpu().numpy()
        img, masks = ctx.render_mesh_masked(dx, du, tex, mvps)
        dark = ctx.render_mesh(dx, du, tb, mvps).cpu().numpy()
    assert (img.cpu().numpy() == plain).all()
    assert (masks.cpu().numpy() == (dark == 0)).all()


def test_mesh_tile_builds_agree():
    """Both tile builds and both binning passes (switches read once per process: one child process each)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = os.path.join(root, "tests", "helpers", "covered_mesh_variants.py")
    outs = []
    for extra in ({}, {"NMI_MESH_NO_PAIRS": "1", "NMI_MESH_NO_SMALL_TILES": "1"}, {"NMI_MESH_NO_PAIRS": "1"}, {"NMI_MESH_NO_SMALL_TILES": "1"}):
        r = subprocess.run([sys.executable, script], capture_output=True, text=True, timeout=600, env=dict(os.environ, **extra))
        assert r.returncode == 0, r.stdout + r.stderr
        lines = [l for l in r.stdout.splitlines() if l.startswith("COVER")]
        assert len(lines) == 2, r.stdout + r.stderr
        outs.append(lines)
    assert all(o == outs[0] for o in outs[1:]), outs


# ---- 8. end to end --------------------------------------------------------------------------------------------------------
def test_end_to_end_partial_cloud_recovers_the_pose():
    """A cloud that covers part of the view, a camera frame whose uncovered area is bright texture: warp_stack_masked +
    render_points_masked + search_grid_covered picks the planted pose and equals the model."""
    w, h, S, Wn = 160, 120, 9, 9
    K = sy.intrinsics(w, h)
    rp = capi.RenderParams(fx=K[0, 0], fy=K[1, 1], cx=K[0, 2], cy=K[1, 2], near_plane=0.5, far_plane=40.0, point_size=3.0)
    rng = np.random.default_rng(5)
    n = 6000
    xyz = np.stack([rng.uniform(-3, 1, n), rng.uniform(-2, 2, n), np.full(n, 8.0)], -1).astype(np.float32)  # left part of the view
    red = (0.2 + 0.6 * (np.sin(xyz[:, 0] * 3) * np.cos(xyz[:, 1] * 2) > 0)).astype(np.float32)
    trans = [(dx, dy, 0.0) for dy in (-0.3, 0.0, 0.3) for dx in (-0.3, 0.0, 0.3)]
    mvps = np.stack([capi.render_mvp(rp, (0, 0, 0), (0, 0, 1), (0, -1, 0), t) for t in trans])
    Ms = sy.warp_homographies(K, (1, 1, Wn), (0.0, 0.0, 0.02))  # rotations about the optical axis; the centre one is the identity
    planted_s, planted_w = 4, Wn // 2
    with capi.NmiContext(w, h) as ctx:
        dx, dr = dev(xyz), dev(red)
        rs, rm = ctx.render_points_masked(dx, dr, mvps, 3.0)
        frame = torch.flip(rs[planted_s], dims=[0]).contiguous().cpu().numpy().copy()
        cov = torch.flip(rm[planted_s], dims=[0]).cpu().numpy() != 0
        tex = rng.integers(120, 256, (h, w)).astype(np.uint8)  # bright texture where the map does not reach
        frame[~cov] = tex[~cov]
        warps, wm = ctx.warp_stack_masked(dev(frame), Ms)
        ratings = torch.zeros((Wn, S), dtype=torch.float32, device="cuda")
        idx, best = ctx.search_grid_covered(rs, rm, warps, wm, ratings)
        rs_h, rm_h, ws_h, wm_h = rs.cpu().numpy(), rm.cpu().numpy(), warps.cpu().numpy(), wm.cpu().numpy()
    assert idx == planted_w * S + planted_s, (idx, best)
    want, wi, wb, _ = cnp.covered_search(rs_h, ws_h, wm_h, rm_h)
    assert (bits(ratings.cpu().numpy()) == bits(want)).all() and (idx, bits(best)) == (wi, bits(wb))
