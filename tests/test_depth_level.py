"""Depth levels (nmi_level_create_depth, nmi_level_create_depth_block, nmi_level_set_depth_shade), GPU tier, 160 x 120, S = 4,
Wn = 4: a depth level run as the fused point cloud, an unfused cloud (point size 6) and the mesh, each plain, masked and covered --
renders, warps and ratings of nmi_level_copy_outputs equal the separate calls (the depth render, nmi_warp_stack[_masked],
nmi_search_grid[_masked|_covered]); the shade set and cleared on levels that have attributes; a block against the whole; and the
planted pose through the deep-frame intake.  `==` on every byte and on the bits of every score.
"""
import ctypes as C

import numpy as np
import pytest

from helpers import depth_np as dn
from helpers import mesh_cases as mc
from helpers import render_cases as rc
from orbslam2_nmi_amd import capi, synthetic as sy

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

f32 = np.float32
W, H, S, WN = 160, 120, 4, 4
SHIFTS = [(-0.06, 0.0, 0.0), (0.0, 0.0, 0.0), (0.05, 0.03, 0.0), (0.02, -0.05, 0.1)]     # view 1 is the centre
CENTRE, PLANTED = 1, 2
SHADE = dn.make(rc.ZN, rc.ZF, 1000.0, 6000, 28000)


@pytest.fixture(scope="module")
def nmi():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    import orbslam2_nmi_amd as m
    m.load_library()
    return m


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(x):
    return np.ascontiguousarray(x, f32).view(np.uint32)


def cshade(sh=SHADE):
    return capi.NmiDepthShade(**sh)


class Scene:
    """A tessellated, tilted mesh (mesh_cases.tessellation_mesh, 40 x 30 quads), the same surface as a cloud (its corners), four
    views around the first of the tessellation's, four warps (the first is the identity), and a grey frame: a depth render from a
    fifth place, rows flipped."""

    def __init__(self, ctx):
        base = mc.tessellation_views(W, H)[:1]
        xyz, _, _ = mc.tessellation_mesh(W, H, base[0], nx=40, ny=30, seed=8)
        self.tri = dev(xyz.astype(f32))
        self.pts = dev(np.unique(xyz.astype(f32), axis=0))
        self.mvps = np.concatenate([rc.shifted(base, t) for t in SHIFTS])
        self.Ms = capi.warp_homographies(sy.intrinsics(W, H), (2, 2, 1), (0.02, 0.02, 0.05))
        assert len(self.Ms) == WN and np.abs(self.Ms[0] - np.eye(3)).max() < 1e-12
        self.Ms[0] = np.eye(3)      # (K I K^-1 in floating point is the identity to a few 1e-15: make it exact)
        fr = ctx.render_mesh_depth(self.tri, rc.shifted(base, (0.01, 0.0, 0.0)), cshade())[0][0]
        self.frame = torch.flip(fr, dims=[0]).contiguous()
        self.fm = dev((np.add.outer(np.arange(H), np.arange(W)) % 7 != 0).astype(np.uint8))     # a frame mask with holes

    def xyz(self, kind):
        return self.tri if kind == "mesh" else self.pts

    def level(self, nmi, ctx, kind, frame=None, block=None, S_=S, Wn_=WN):
        size = {"fused": 3.0, "unfused": 6.0, "mesh": 1.0}[kind]
        return nmi.NmiLevel(ctx, self.xyz(kind), None, self.frame if frame is None else frame, S_, Wn_, size, depth=cshade(),
                            mesh=kind == "mesh", block=block)

    def render(self, ctx, kind, mvps=None):
        """The separate call -> (grey, masks) device tensors."""
        mvps = self.mvps if mvps is None else mvps
        if kind == "mesh":
            g, m, _ = ctx.render_mesh_depth(self.tri, mvps, cshade(), out_masks=True)
        else:
            g, m, _ = ctx.render_points_depth(self.pts, None, mvps, 3.0 if kind == "fused" else 6.0, cshade(), out_masks=True)
        return g, m


def search(ctx, mode, rs, rm, ws, wm):
    t = torch.full((ws.shape[0], rs.shape[0]), -3.0, device="cuda")
    if mode == "plain":
        win = ctx.search_grid(rs, ws, t)
    elif mode == "masked":
        win = ctx.search_grid_masked(rs, ws, wm, t)
    else:
        win = ctx.search_grid_covered(rs, rm, ws, wm, t)
    return win, t.cpu().numpy()


@pytest.mark.parametrize("mode", ["plain", "masked", "covered"])
@pytest.mark.parametrize("kind", ["fused", "unfused", "mesh"])
def test_depth_level_equals_separate_calls(nmi, kind, mode):
    with nmi.NmiContext(W, H) as ctx:
        sc = Scene(ctx)
        rs, rm = sc.render(ctx, kind)
        assert 0 < int(rm.sum()) < rm.numel(), "the premise: part of every stack is covered, part is not"
        assert len(torch.unique(rs)) > 64
        if mode == "plain":
            ws, wm = ctx.warp_stack(sc.frame, sc.Ms), None
        else:
            ws, wm = ctx.warp_stack_masked(sc.frame, sc.Ms, sc.fm)
        want, table = search(ctx, mode, rs, rm, ws, wm)
        assert len(np.unique(table)) > S * WN // 2, "the ratings do not tell the cells apart"
        with sc.level(nmi, ctx, kind) as lv:
            if mode == "masked":
                lv.set_masks(True, sc.fm)
            if mode == "covered":
                lv.set_coverage(True, sc.fm)
            for rep in range(2):
                got = lv.run(sc.mvps, sc.Ms)
                r, v, t = lv.outputs()
                assert (r == rs.cpu().numpy()).all(), f"replay {rep}: {(r != rs.cpu().numpy()).sum()} render bytes differ"
                assert (v == ws.cpu().numpy()).all()
                assert (bits(t) == bits(table)).all()
                assert got[0] == want[0] and bits(got[1]) == bits(want[1]), (got, want)
                if mode == "masked":
                    assert (lv.masks()[0] == wm.cpu().numpy()).all()
                if mode == "covered":
                    cov = lv.coverage()
                    assert (cov[0] == rm.cpu().numpy()).all() and (cov[1] == wm.cpu().numpy()).all()
            # other views: the level follows
            moved = rc.shifted(sc.mvps, (0.07, -0.05, 0.3))
            lv.run(moved, sc.Ms)
            assert (lv.outputs()[0] == sc.render(ctx, kind, moved)[0].cpu().numpy()).all()
            with pytest.raises(nmi.NmiError):
                lv.set_depth_shade(None)            # created without attributes: no colour to go back to
            lv.run(sc.mvps, sc.Ms)
            assert (lv.outputs()[0] == rs.cpu().numpy()).all()


@pytest.mark.parametrize("kind", ["cloud", "colored_mesh", "textured_mesh"])
def test_set_depth_shade_and_back(nmi, kind):
    """On a level that has attributes: the shade gives the depth render, NULL returns the original bytes -- renders and ratings."""
    with nmi.NmiContext(W, H) as ctx:
        sc = Scene(ctx)
        rng = np.random.default_rng(5)
        tex = None
        if kind == "cloud":
            xyz, attr = sc.pts, dev(rng.uniform(0, 1, len(sc.pts)).astype(f32))
            lv = nmi.NmiLevel(ctx, xyz, attr, sc.frame, S, WN, 3.0)
            depth = ctx.render_points_depth(xyz, attr, sc.mvps, 3.0, cshade())[0]
        elif kind == "colored_mesh":
            xyz, attr = sc.tri, dev(rng.uniform(0, 1, len(sc.tri)).astype(f32))
            lv = nmi.NmiLevel(ctx, xyz, attr, sc.frame, S, WN, 1.0, colors=True)
            depth = ctx.render_mesh_depth(xyz, sc.mvps, cshade())[0]
        else:
            xyz, attr = sc.tri, dev(rng.uniform(0, 1, (len(sc.tri), 2)).astype(f32))
            tex = nmi.NmiTexture(ctx, rng.integers(0, 256, (16, 16, 3), dtype=np.uint8))
            lv = nmi.NmiLevel(ctx, xyz, attr, sc.frame, S, WN, 1.0, texture=tex)
            depth = ctx.render_mesh_depth(xyz, sc.mvps, cshade())[0]
        with lv:
            first = lv.run(sc.mvps, sc.Ms)
            r0, _, t0 = lv.outputs()
            assert not (r0 == depth.cpu().numpy()).all()
            bad = cshade(dict(SHADE, lo=SHADE["hi"]))
            assert lv._lib.nmi_level_set_depth_shade(lv._h, C.byref(bad)) == capi.ERR_INVALID_ARGUMENT      # refused: the level as it was
            assert lv.run(sc.mvps, sc.Ms) == first and (lv.outputs()[0] == r0).all()
            lv.set_depth_shade(cshade())
            lv.run(sc.mvps, sc.Ms)
            assert (lv.outputs()[0] == depth.cpu().numpy()).all()
            lv.set_depth_shade(None)
            again = lv.run(sc.mvps, sc.Ms)
            r1, _, t1 = lv.outputs()
            assert (r1 == r0).all() and (bits(t1) == bits(t0)).all()
            assert again[0] == first[0] and bits(again[1]) == bits(first[1])
        if tex is not None:
            tex.close()


@pytest.mark.parametrize("kind", ["fused", "mesh"])
def test_depth_block_equals_its_slice(nmi, kind):
    with nmi.NmiContext(W, H) as ctx:
        sc = Scene(ctx)
        with sc.level(nmi, ctx, kind) as whole:
            whole.run(sc.mvps, sc.Ms)
            table = whole.outputs()[2]
        s0, s1, w0, w1 = 1, 4, 1, 3
        with sc.level(nmi, ctx, kind, block=(s0, S, w0, WN), S_=s1 - s0, Wn_=w1 - w0) as blk:
            got = blk.run(sc.mvps[s0:s1], sc.Ms[w0:w1])
            t = blk.outputs()[2]
            cells = table[w0:w1, s0:s1]
            assert (bits(t) == bits(cells)).all()
            best = cells.max()
            ww, ss = np.nonzero(cells == best)
            index = int(min((w0 + a) * S + (s0 + b) for a, b in zip(ww, ss)))
            assert got[0] == index and bits(got[1]) == bits(best), (got, index, best)


def test_planted_pose(nmi):
    """The frame is the row-flipped depth16 of view PLANTED of the mesh, read as GRAY16 under NMI_TONE_WINDOW(lo, hi) and the valid
    range (1, 65535); the level is the depth level with that window, masked by validity alone.  The winner is (identity warp,
    PLANTED) and its score is the self-score of that render, taken by the separate calls."""
    with nmi.NmiContext(W, H) as ctx:
        sc = Scene(ctx)
        g, m, d16 = ctx.render_mesh_depth(sc.tri, sc.mvps, cshade(), out_masks=True, depth16=True)
        assert 0 < int(m[PLANTED].sum()) < m[PLANTED].numel()
        raw = torch.flip(d16[PLANTED], dims=[0]).contiguous()
        frame = raw.view(torch.uint8)       # [H][2 W] bytes: the GRAY16 frame, dense
        # the self-score: the render against itself, through the standalone masked chain
        own = torch.flip(g[PLANTED], dims=[0]).contiguous()
        own_mask = torch.flip(m[PLANTED], dims=[0]).contiguous()
        ws, wm = ctx.warp_stack_masked(own, sc.Ms[:1], own_mask)
        self_score = ctx.search_grid_masked(g[PLANTED:PLANTED + 1], ws, wm)[1]
        with sc.level(nmi, ctx, "mesh", frame=frame) as lv:
            lv.set_frame_format(capi.FRAME_GRAY16)
            lv.set_tone_map(capi.ToneMap.window(SHADE["lo"], SHADE["hi"], bits=16))
            lv.set_valid_range(1, 65535)
            lv.set_masks(True)
            index, score = lv.run(sc.mvps, sc.Ms)
            r, v, t = lv.outputs()
            assert (r == g.cpu().numpy()).all()
            cov = own_mask.cpu().numpy() != 0
            assert (v[0][cov] == own.cpu().numpy()[cov]).all(), "the intake's grey differs from the render's on covered pixels"
            assert (lv.masks()[0][0] == wm.cpu().numpy()[0]).all()
            assert PLANTED != CENTRE and index == 0 * S + PLANTED, (index, t)
            assert bits(score) == bits(self_score), (score, self_score)
            assert (t.reshape(-1)[np.arange(S * WN) != index] < score).all()
