"""The twin and the float64 model of the depth shade (include/nmi_hip.h, "Depth maps"; csrc/nmi_depth_device.h) -- TEST
INFRASTRUCTURE ONLY.

The rule, for a pixel whose winner has the 24-bit window depth d, in fp32 with every operation rounded on its own:
    u    = (float)(2^24 - 1 - d) / (2^24 - 1)
    den  = near + u (far - near)
    z    = (near far) / den
    v    = clamp((uint32)(z scale + 0.5), 1, 65535)
    grey = v <= lo: 0; v >= hi: 255; else ((v - lo) 255 + ((hi - lo) >> 1)) // (hi - lo)        (NMI_TONE_WINDOW's integer rule)
and v = 0, grey = 255 where nothing won.  numpy's float32 arithmetic is IEEE and never fused, so shade() below is the bytes the
device must produce; shade_f64() is the same formula in float64.  No rasteriser here: the depths come from the committed oracles
(oracle/render_oracle_np.render_keys(...) >> 8 with EMPTY, oracle/mesh_oracle_np.render_staged(...)["depth"] with EMPTY_DEPTH).
"""
import numpy as np

from oracle import mesh_oracle_np as mo
from oracle import render_oracle_np as ro

f32 = np.float32
D_MAX = 0xFFFFFF


def make(near, far, scale, lo, hi):
    """A shade as a plain dict (the tests build the C struct from it: NmiDepthShade(**shade))."""
    return {"near_plane": float(f32(near)), "far_plane": float(f32(far)), "scale": float(f32(scale)), "lo": int(lo), "hi": int(hi)}


def window_rule(v, lo, hi):
    v = np.asarray(v, np.int64)
    mid = ((v - lo) * 255 + ((hi - lo) >> 1)) // (hi - lo)
    return np.where(v <= lo, 0, np.where(v >= hi, 255, mid)).astype(np.uint8)


def raw_depth(d, shade, F=f32):
    """v of the depths d (any integer array, values 0 .. 2^24 - 1) in the float type F -> int64 array."""
    d = np.asarray(d, np.int64)
    near, far, scale = F(f32(shade["near_plane"])), F(f32(shade["far_plane"])), F(f32(shade["scale"]))
    with np.errstate(all="ignore"):
        u = (D_MAX - d).astype(F) / F(16777215.0)
        den = near + u * (far - near)
        z = (near * far) / den
        x = z * scale + F(0.5)
        return np.fmin(np.fmax(x, F(1.0)), F(65535.0)).astype(np.int64)     # truncation; the clamp on the float, as the kernel


def shade(d, shade_, empty=None, F=f32):
    """-> (v uint16, grey uint8) of the depths d; where d == empty (if given): v = 0, grey = 255."""
    d = np.asarray(d, np.int64)
    nothing = (d == empty) if empty is not None else np.zeros(d.shape, bool)
    v = raw_depth(np.where(nothing, 0, d), shade_, F)
    grey = window_rule(v, shade_["lo"], shade_["hi"])
    return np.where(nothing, 0, v).astype(np.uint16), np.where(nothing, 255, grey).astype(np.uint8)


def shade_f64(d, shade_):
    return shade(d, shade_, F=np.float64)


def points_view(xyz, red, mvp, W, H, point_size, shade_):
    """One view of a cloud -> (grey [H, W] u8, v [H, W] u16, covered [H, W] u8), bottom-up rows.  red None: colour 0."""
    red = np.zeros(len(xyz), f32) if red is None else red
    keys = ro.render_keys(xyz, red, mvp, W, H, point_size).astype(np.int64)
    v, grey = shade(np.where(keys == int(ro.EMPTY), -1, keys >> 8), shade_, empty=-1)
    return grey.reshape(H, W), v.reshape(H, W), (keys != int(ro.EMPTY)).astype(np.uint8).reshape(H, W)


def points_stack(xyz, red, mvps, W, H, point_size, shade_):
    views = [points_view(xyz, red, m, W, H, point_size, shade_) for m in np.asarray(mvps, f32).reshape(-1, 16)]
    return tuple(np.stack([t[k] for t in views]) for k in range(3))


def mesh_view(staged, shade_):
    """One view of a mesh from render_staged's (or helpers/mesh_color.render's) result -> (grey, v, covered) as points_view."""
    depth = np.asarray(staged["depth"], np.int64)
    v, grey = shade(depth, shade_, empty=mo.EMPTY_DEPTH)
    covered = np.asarray(staged["covered"], bool)
    assert ((depth != mo.EMPTY_DEPTH) == covered).all()
    return grey, v, covered.astype(np.uint8)


def mesh_stack(staged_views, shade_):
    views = [mesh_view(s, shade_) for s in staged_views]
    return tuple(np.stack([t[k] for t in views]) for k in range(3))
