"""GPU tests (-m gpu) of levels fed full-size frames (nmi_level_set_frame_reduction).

The contract: a level whose frame is a full-size camera frame equals the standalone chain on that frame -- nmi_reduce_frame ->
[nmi_undistort_frame] -> nmi_warp_stack[_masked] -> render -> nmi_search_grid[_masked / _covered] -- on == of ratings bits,
winner, warps, warp masks and counts.  Also: the frame is read in place on every replay, masks / coverage / distortion set in any
order keep the reduction, of nmi_level_set_frame_format and nmi_level_set_frame_reduction the later call wins, turning it off gives
the bytes of a never-set level, and a refused call leaves the level as it was."""
import numpy as np
import pytest

from helpers import color_np as cnp
from helpers import covered_np as covnp
from helpers import reduce_np as rnp
from helpers import undistort_np as unp
from orbslam2_nmi_amd import capi
from test_color_level import bits, enable, lens_K, scene
from test_covered_level import CoveredScene
from test_masked_level import dev, hood_mask, views, warps

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

LENSES = {"none": None, "barrel": unp.FAMILIES["barrel"]}


@pytest.fixture(scope="module")
def nmi():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    import orbslam2_nmi_amd as m
    m.load_library()
    return m


def full_size(gray, f, seed=0):
    """[H,W] grey -> [f*H, f*W] grey: each pixel spread over its f x f block with a fine texture on top, so that the blocks are
    not constant and the reduced frame is about the input."""
    rng = np.random.default_rng(seed)
    big = np.kron(gray.astype(np.int64), np.ones((f, f), np.int64))
    return np.clip(big + rng.integers(-9, 10, big.shape), 0, 255).astype(np.uint8)


class FullFrame:
    """The scene's grey frame at f times its size (full_size), coloured for a colour format (helpers/color_np.py: colorize) and laid
    out in fmt with a pitch, `off` bytes into a device allocation.  .view is the frame's first byte onwards: the level's d_frame."""

    def __init__(self, sc, f, fmt, pitch, off, seed=0):
        self.f, self.fmt, self.pitch, self.off = f, fmt, pitch, off
        self.w, self.h = sc.w, sc.h
        self.buf = dev(self.layout(full_size(sc.frame.cpu().numpy(), f, seed), seed))
        self.view = self.buf[off:]

    def layout(self, big, seed):
        self.big = big
        img = big if self.fmt == cnp.GRAY else cnp.colorize(big, seed)
        return cnp.pack(img, self.fmt, self.pitch, self.off, seed=seed)

    def refill(self, big, seed):
        """New contents in place (the same addresses)."""
        self.buf.copy_(dev(self.layout(big, seed)))
        torch.cuda.synchronize()

    def twin(self):
        return rnp.reduce_frame(self.buf.cpu().numpy(), self.fmt, self.w, self.h, self.f, self.pitch, self.off)


def level(nmi, sc, ff, S, Wn):
    return nmi.NmiLevel(sc.ctx, sc.dx, sc.da, ff.view, S, Wn, 3.0, texture=sc.tex)


def rest_of_chain(ctx, sc, gray, kind, K, dist, fm, mvps, Ms, rs):
    """[nmi_undistort_frame] -> warps -> search on a grey frame of the search size -> (winner, ratings, warps, warp masks or None)."""
    t2 = torch.full((len(Ms), len(mvps)), -3.0, device="cuda")
    if kind == "plain":
        frame = gray if dist is None else ctx.undistort_frame(gray, K, dist, out_mask=False)[0]
        ws = ctx.warp_stack(frame, Ms)
        win = ctx.search_grid(dev(rs), ws, t2)
        return win, t2.cpu().numpy(), ws.cpu().numpy(), None
    frame, fmask = (gray, fm) if dist is None else ctx.undistort_frame(gray, K, dist, raw_mask=fm)
    ws, wm = ctx.warp_stack_masked(frame, Ms, fmask)
    if kind == "masked":
        win = ctx.search_grid_masked(dev(rs), ws, wm, t2)
    else:
        rs2, rm2 = sc.chain_renders(ctx, mvps)
        assert (rs2.cpu().numpy() == rs).all()
        win = ctx.search_grid_covered(rs2, rm2, ws, wm, t2)
    return win, t2.cpu().numpy(), ws.cpu().numpy(), wm.cpu().numpy()


def check_against(ctx, sc, gray, lv, kind, K, dist, fm, mvps, Ms):
    """One replay of lv against the chain on the grey frame `gray` -> (winner, ratings)."""
    win = lv.run(mvps, Ms)
    rs, ws, t = lv.outputs()
    cw, ct, cws, cwm = rest_of_chain(ctx, sc, gray, kind, K, dist, fm, mvps, Ms, rs)
    assert (cws == ws).all(), "level warps != warps of the chain's frame"
    assert cw == win and (bits(ct) == bits(t)).all(), (cw, win)
    if kind == "masked":
        wm, cnt = lv.masks()
        assert (wm == cwm).all()
        assert (cnt == np.count_nonzero(cwm.reshape(len(Ms), -1), axis=1)).all()
    if kind == "covered":
        rm, wm, cnt = lv.coverage()
        assert (wm == cwm).all()
        assert (rm == sc.chain_renders(ctx, mvps)[1].cpu().numpy()).all()
        assert (ctx.cover_counts(t.size).reshape(t.shape) == cnt).all()   # (of the chain's covered search, the latest on ctx)
        assert (cnt == covnp.cover_counts(wm, rm)).all()
    return win, t


def check(ctx, sc, ff, lv, kind, K, dist, fm, mvps, Ms):
    gray = ctx.reduce_frame(ff.view, ff.fmt, ff.f, ff.pitch)
    assert (gray.cpu().numpy() == ff.twin()).all()
    return check_against(ctx, sc, gray, lv, kind, K, dist, fm, mvps, Ms)


# search size, factor, format, extra pitch bytes, base offset: f = 2 RGB pitched (16-byte loads), f = 4 grey dense off an odd base
CASES = [(424, 240, 2, cnp.RGB, 16, 0), (160, 120, 4, cnp.GRAY, None, 3)]


def make(sc, case, seed=0):
    w, h, f, fmt, extra, off = case
    pitch = 0 if extra is None else f * w * cnp.BPP[fmt] + extra
    return FullFrame(sc, f, fmt, pitch, off, seed)


@pytest.mark.parametrize("lens", list(LENSES))
@pytest.mark.parametrize("kind", ["plain", "masked", "covered"])
@pytest.mark.parametrize("mesh", [False, True], ids=["cloud", "mesh"])
@pytest.mark.parametrize("case", CASES, ids=["424x240-f2-rgb-pitched", "160x120-f4-gray"])
def test_reduced_level_equals_the_chain(nmi, case, mesh, kind, lens):
    """Reduction set before and after the masks and the distortion (three orders); replays with changed views and warps; the
    full-size frame's contents replaced in place."""
    w, h, f = case[:3]
    S, Wn = 3, 3
    dist = LENSES[lens]
    with nmi.NmiContext(w, h) as ctx:
        sc = scene(nmi, ctx, w, h, mesh, kind)
        K = lens_K(sc.rp)
        ff = make(sc, case)
        fm = dev(hood_mask(w, h)) if kind != "plain" else None      # dense [H][W], at the search size
        mvps, Ms = views(sc.rp, S), warps(w, h, Wn)
        with level(nmi, sc, ff, S, Wn) as lv, level(nmi, sc, ff, S, Wn) as lv2, level(nmi, sc, ff, S, Wn) as lv3:
            lv.set_frame_reduction(ff.f, ff.fmt, ff.pitch)           # reduction, distortion, masks
            if dist is not None:
                lv.set_distortion(K, dist)
            enable(lv, kind, fm)
            enable(lv2, kind, fm)                                    # masks, distortion, reduction
            if dist is not None:
                lv2.set_distortion(K, dist)
            lv2.set_frame_reduction(ff.f, ff.fmt, ff.pitch)
            if dist is not None:                                     # distortion, reduction, masks
                lv3.set_distortion(K, dist)
            lv3.set_frame_reduction(ff.f, ff.fmt, ff.pitch)
            enable(lv3, kind, fm)
            first = check(ctx, sc, ff, lv, kind, K, dist, fm, mvps, Ms)
            for other in (lv2, lv3):
                again = check(ctx, sc, ff, other, kind, K, dist, fm, mvps, Ms)
                assert again[0] == first[0] and (bits(again[1]) == bits(first[1])).all()
            check(ctx, sc, ff, lv, kind, K, dist, fm, views(sc.rp, S, 1.7), warps(w, h, Wn, 1.6))
            ff.refill(np.roll(ff.big, shift=(7 * f, 11 * f + 1), axis=(0, 1)), seed=1)   # the frame changes in place
            if fm is not None:
                fm[h // 3:h // 2, w // 3:w // 2] = 0
                torch.cuda.synchronize()
            moved = check(ctx, sc, ff, lv, kind, K, dist, fm, mvps, Ms)
            assert (bits(moved[1]) != bits(first[1])).any()


@pytest.mark.parametrize("mesh", [False, True], ids=["cloud", "mesh"])
def test_later_call_wins_off_restores_and_refusals_change_nothing(nmi, mesh):
    """set_frame_format after set_frame_reduction wins, and the reverse; (1, GRAY, 0) and set_frame_format(GRAY, 0) restore the
    graph: bytes == a level on the same buffer that never had a setting, with and without distortion; toggling masks and coverage
    in between keeps the reduction.  Rejected calls leave the level as it was."""
    w, h, S, Wn, f = 320, 240, 3, 3, 2
    with nmi.NmiContext(w, h) as ctx:
        sc = CoveredScene(nmi, ctx, w, h, mesh)
        K = lens_K(sc.rp)
        ff = FullFrame(sc, f, cnp.RGBA, f * w * 4 + 64, 0)
        mvps, Ms = views(sc.rp, S), warps(w, h, Wn)
        lens = LENSES["barrel"]
        with level(nmi, sc, ff, S, Wn) as lv, level(nmi, sc, ff, S, Wn) as never, level(nmi, sc, ff, S, Wn) as never_d:
            never_d.set_distortion(K, lens)
            refs = {}
            for name, ref in (("plain", never), ("distorted", never_d)):
                refs[name] = (ref.run(mvps, Ms), ref.outputs())

            def same_as(name):
                win, out = refs[name]
                assert lv.run(mvps, Ms) == win
                for a, b in zip(lv.outputs(), out):
                    assert (np.ascontiguousarray(a).view(np.uint8) == np.ascontiguousarray(b).view(np.uint8)).all()

            def reduced(kind="plain", dist=None):
                return check(ctx, sc, ff, lv, kind, K, dist, None, mvps, Ms)

            def formatted(fmt, pitch, dist=None):
                """The level as set_frame_format(fmt, pitch) leaves it: the buffer's first H rows of W pixels."""
                gray = ctx.gray_frame(ff.view, fmt, pitch)
                return check_against(ctx, sc, gray, lv, "plain", K, dist, None, mvps, Ms)

            lv.set_frame_reduction(f, ff.fmt, ff.pitch)
            base = reduced()
            for bad in ((0, ff.fmt, ff.pitch), (5, ff.fmt, ff.pitch), (-2, ff.fmt, 0), (f, 9, 0), (f, ff.fmt, 1), (f, ff.fmt, f * w * 4 - 1),
                        (f, ff.fmt, w * 4), (f, cnp.RGB, -3)):
                with pytest.raises(capi.NmiError):
                    lv.set_frame_reduction(*bad)
            with pytest.raises(capi.NmiError):
                lv.set_frame_format(9, 0)
            after = reduced()                                              # as it was
            assert after[0] == base[0] and (bits(after[1]) == bits(base[1])).all()
            lv.set_masks(True)
            reduced("masked")
            lv.set_masks(False)
            lv.set_coverage(True)
            reduced("covered")
            lv.set_coverage(False)
            lv.set_frame_format(cnp.BGRA, ff.pitch)                        # the later call wins: a frame of the search size
            formatted(cnp.BGRA, ff.pitch)
            lv.set_frame_reduction(f, ff.fmt, ff.pitch)                    # ... and the reverse
            reduced()
            lv.set_frame_reduction(1, cnp.BGRA, ff.pitch)                  # factor 1 is set_frame_format exactly
            formatted(cnp.BGRA, ff.pitch)
            lv.set_frame_reduction(f, ff.fmt, ff.pitch)
            lv.set_frame_reduction(1, cnp.GRAY, 0)                         # off
            same_as("plain")
            lv.set_frame_reduction(f, ff.fmt, ff.pitch)
            lv.set_distortion(K, lens)
            reduced(dist=lens)
            lv.set_frame_format(cnp.GRAY, 0)                               # off through the other call
            same_as("distorted")
            lv.set_frame_reduction(f, ff.fmt, ff.pitch)
            lv.set_frame_format(cnp.BGRA, ff.pitch)                        # the fused colour node, after a reduced distorted graph
            formatted(cnp.BGRA, ff.pitch, lens)
            lv.set_frame_reduction(f, ff.fmt, ff.pitch)
            lv.set_distortion(None, None)                                  # distortion off keeps the reduction
            after = reduced()
            assert after[0] == base[0] and (bits(after[1]) == bits(base[1])).all()
            lv.set_frame_reduction(1, cnp.GRAY, w)
            same_as("plain")
