"""Renders a mesh with nmi_render_mesh_masked and checks it against nmi_render_mesh and a black-texture render, then prints a
hash of the masks.  Run by tests/test_covered_render.py once per choice of the renderer's tile builds (environment switches
the library reads once per process): the checks must hold and the hashes must not depend on the choice."""
import hashlib
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import orbslam2_nmi_amd as nmi
from orbslam2_nmi_amd import capi, synthetic as sy
w, h = 848, 480
K = sy.intrinsics(w, h)
rp = capi.RenderParams(fx=K[0, 0], fy=K[1, 1], cx=K[0, 2], cy=K[1, 2], near_plane=5.0, far_plane=30.0, point_size=1.0)
B = sy.scene(256, 256, 5)
rgb = np.stack([B, B, B], -1).astype(np.uint8)
black = np.zeros_like(rgb)
for nx, ny, S in ((40, 30, 27), (400, 300, 27)):
    rng = np.random.default_rng(nx)
    mvps = np.stack([capi.render_mvp(rp, (0, 0, 0), (0, 0, 1), (0, 1, 0), tuple(rng.uniform(-0.4, 0.4, 3))) for _ in range(S)])
    # a relief covering part of the view only (the quads span the middle of the image), both windings
    us, vs = np.linspace(0.2 * w, 0.8 * w, nx + 1), np.linspace(0.1 * h, 0.9 * h, ny + 1)
    uu, vv = np.meshgrid(us, vs)
    z = 10.0 + 2.0 * np.sin(uu * 0.01) * np.cos(vv * 0.013)
    P = np.stack([(uu - rp.cx) / rp.fx * z, (vv - rp.cy) / rp.fy * z, z], -1).astype(np.float32)
    T = np.stack([uu / w, vv / h], -1).astype(np.float32)
    p00, p10, p01, p11 = P[:-1, :-1], P[:-1, 1:], P[1:, :-1], P[1:, 1:]
    t00, t10, t01, t11 = T[:-1, :-1], T[:-1, 1:], T[1:, :-1], T[1:, 1:]
    xyz = np.concatenate([np.stack([p00, p10, p11, p00, p11, p01], 2).reshape(-1, 3), np.stack([p00, p11, p10, p00, p01, p11], 2).reshape(-1, 3)])
    uv = np.concatenate([np.stack([t00, t10, t11, t00, t11, t01], 2).reshape(-1, 2), np.stack([t00, t11, t10, t00, t01, t11], 2).reshape(-1, 2)])
    dx, du = torch.from_numpy(np.ascontiguousarray(xyz)).cuda(), torch.from_numpy(np.ascontiguousarray(uv)).cuda()
    with nmi.NmiContext(w, h) as ctx, nmi.NmiTexture(ctx, rgb) as tex, nmi.NmiTexture(ctx, black) as tb:
        plain = ctx.render_mesh(dx, du, tex, mvps).cpu().numpy()
        img, masks = ctx.render_mesh_masked(dx, du, tex, mvps)
        dark = ctx.render_mesh(dx, du, tb, mvps).cpu().numpy()
        img, masks = img.cpu().numpy(), masks.cpu().numpy()
    assert (img == plain).all(), "masked render differs from nmi_render_mesh"
    assert set(np.unique(dark)) <= {0, 255}
    assert (masks == (dark == 0)).all(), f"{(masks != (dark == 0)).sum()} mask pixels differ"
    cov = float(masks.mean())
    assert 0.05 < cov < 0.95, cov
    print("COVER", nx, ny, S, round(cov, 3), hashlib.sha256(masks.tobytes()).hexdigest()[:16])
