"""numpy (fp32) restatement of the point-cloud render-stack producer -- TEST INFRASTRUCTURE ONLY.

Restates Rendering<4>::renderToTextureOnGPU (Thirdparty/Localization/rendering.hpp:530-630) + shaders/ShadingWithColor.*:
clear colour 1.0 (:533), gl_Position = MVP * vec4(p, 1), GL_POINTS of glPointSize (:307), depth test GL_LESS (:294-297),
red channel into a GL_RED 8-bit texture (:347).  The rasteriser belongs to the OpenGL driver, which the reference does
not contain; the point rules are those of the OpenGL 3.3 specification (section 3.4.1, non-antialiased points) and a
24-bit depth buffer.  "PARITY UNPINNED": nothing in the reference tree (and no GL here) to check these pixels against.
"""
import numpy as np

f32 = np.float32


def look_at(eye, center, up):
    """glm::lookAt (right-handed), float64 model used only to cross-check the product's fp32 matrix."""
    eye, center, up = (np.asarray(v, np.float64) for v in (eye, center, up))
    f = center - eye
    f /= np.linalg.norm(f)
    s = np.cross(f, up)
    s /= np.linalg.norm(s)
    u = np.cross(s, f)
    V = np.eye(4)
    V[0, :3], V[1, :3], V[2, :3] = s, u, -f
    V[0, 3], V[1, 3], V[2, 3] = -s @ eye, -u @ eye, f @ eye
    return V


def projection(fx, fy, cx, cy, zn, zf):
    """rendering.hpp:196-202 (glm columns written out as a conventional row-major 4x4)."""
    P = np.zeros((4, 4))
    P[0, 0] = fx / (-cx)
    P[1, 1] = fy / (-cy)
    P[2, 2] = (zn + zf) / (zn - zf)
    P[3, 2] = -1.0
    P[2, 3] = 2 * zn * zf / (zn - zf)
    return P


MAX_POINT_SIZE = 64
DEPTH_MAX = (1 << 24) - 1      # the largest 24-bit depth: the far plane
EMPTY = np.uint32(0xFFFFFFFF)   # an anchor no point reached (the clear colour 255 at depth "beyond the far plane")


def point_size_rule(point_size):
    """glPointSize for non-antialiased points as the product applies it (include/nmi_hip.h, nmi_render_points): NaN is
    rejected (ValueError here, NMI_ERR_INVALID_ARGUMENT there); otherwise floor(size + 0.5) in fp32, clamped to [1, 64] in
    float before any conversion to int, so 1e10 and inf give 64 (GL clamps to the largest supported size)."""
    p = f32(point_size)
    if np.isnan(p):
        raise ValueError("point_size is NaN")
    with np.errstate(over="ignore"):
        s = np.floor(p + f32(0.5))
    return int(min(max(s, f32(1.0)), f32(MAX_POINT_SIZE)))


def sprite_origin(xw, size):
    """Lowest-left pixel of the size x size sprite of window coordinate xw (any float dtype): odd sizes are centred on
    floor(xw) + 0.5, even sizes on floor(xw + 0.5)."""
    if size & 1:
        return np.floor(xw).astype(np.int64) - (size - 1) // 2
    return np.floor(xw + xw.dtype.type(0.5)).astype(np.int64) - size // 2


def clip_fp32(xyz, mvp_colmajor):
    """-> cx, cy, cz, cw [N] float32: glm mat4 * vec4 as splat_anchor sums it, c_r = (m[r] x + m[4+r] y) + (m[8+r] z + m[12+r])."""
    m = np.asarray(mvp_colmajor, f32).reshape(16)
    x, y, z = (np.asarray(xyz, f32).reshape(-1, 3)[:, k] for k in range(3))
    with np.errstate(over="ignore", invalid="ignore"):
        return tuple((m[r] * x + m[4 + r] * y) + (m[8 + r] * z + m[12 + r]) for r in range(4))


def window_fp32(xyz, mvp_colmajor, width, height):
    """-> xw, yw, zw [N] float32 as splat_anchor computes them (meaningful where point_fragments keeps the point)."""
    cx, cy, cz, cw = clip_fp32(xyz, mvp_colmajor)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        iw = f32(1.0) / cw
        return ((cx * iw * f32(0.5) + f32(0.5)) * f32(width), (cy * iw * f32(0.5) + f32(0.5)) * f32(height),
                cz * iw * f32(0.5) + f32(0.5))


def point_fragments(xyz, red, mvp_colmajor, width, height, size):
    """One view, per point, in fp32 exactly as splat_anchor (csrc/nmi_cloud_device.h) computes it.
    -> keep [N] bool, x0, y0 [N] int64 (sprite origin), depth [N] uint32 (24 bits), colour [N] uint32 (8 bits); x0 .. colour
    are 0 where keep is False.  keep: cw a positive normal float and |cx|, |cy|, |cz| <= cw (NaN fails every comparison)."""
    n = len(np.asarray(xyz).reshape(-1, 3))
    cx, cy, cz, cw = clip_fp32(xyz, mvp_colmajor)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        normal = (cw >= np.finfo(f32).tiny) & (cw <= np.finfo(f32).max)
        keep = normal & (np.abs(cx) <= cw) & (np.abs(cy) <= cw) & (np.abs(cz) <= cw)
        cx, cy, cz, cw = (np.where(keep, c, f32(1.0)) for c in (cx, cy, cz, cw))
        iw = f32(1.0) / cw                                  # the perspective divide as one reciprocal and three products
        xw = (cx * iw * f32(0.5) + f32(0.5)) * f32(width)
        yw = (cy * iw * f32(0.5) + f32(0.5)) * f32(height)
        zw = cz * iw * f32(0.5) + f32(0.5)
        q = np.trunc(zw * f32(16777215.0) + f32(0.5))      # (uint32_t) truncates; below 0 it gives 0
    depth = np.minimum(np.maximum(q, 0), DEPTH_MAX).astype(np.uint32)   # at zw = 1 the fp32 sum rounds up to 2^24
    r = np.asarray(red, f32).reshape(-1)
    colour = (np.fmin(np.fmax(r, f32(0.0)), f32(1.0)) * f32(255.0) + f32(0.5)).astype(np.uint32)   # fmaxf / fminf: NaN -> 0
    x0, y0 = sprite_origin(xw, size), sprite_origin(yw, size)
    z0 = np.zeros(n, np.int64)
    return (keep, np.where(keep, x0, z0), np.where(keep, y0, z0), np.where(keep, depth, np.uint32(0)).astype(np.uint32),
            np.where(keep, colour, np.uint32(0)).astype(np.uint32))


def point_fragments_f64(xyz, red, mvp_colmajor, width, height, size):
    """The float64 model of the same rule (same fp32 inputs; every clip, window, depth and colour value in float64):
      keep iff cw > 0 and |cx|, |cy|, |cz| <= cw, NaN not drawn;
      the sprite: the pixels whose centres lie in [c - size/2, c + size/2) on each axis, c = floor(xw) + 0.5 for odd sizes and
      floor(xw + 0.5) for even sizes (OpenGL 3.3, 3.4.1; _gl_square_first_pixel, independent of the twin's sprite_origin);
      depth = min(round(zw * (2^24 - 1)), 2^24 - 1) (round half up), colour = round(clamp(red, 0, 1) * 255), a NaN red -> 0.
    A pixel then keeps the smallest key depth << 8 | colour over the sprites covering it (scatter_min): among equal quantised
    depths the SMALLER red wins, where GL_LESS would keep the point drawn first -- a deliberate deviation of the product (one
    atomicMin per point and view), which this model follows.  A second deliberate deviation: GL clears the depth buffer to 1.0
    and tests LESS, so it draws no point at the far plane; the product draws it at depth 2^24 - 1, behind everything else, and
    only a key of 0xFFFFFFFF (such a point with colour 255) equals an untouched pixel: it shows 255 and is not covered.
    -> keep, x0, y0, depth, colour as point_fragments."""
    m = np.asarray(mvp_colmajor, f32).reshape(16).astype(np.float64)
    P = np.asarray(xyz, f32).reshape(-1, 3).astype(np.float64)
    n = len(P)
    M = m.reshape(4, 4).T                                   # conventional row-major
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        c = P @ M[:, :3].T + M[:, 3]
        cx, cy, cz, cw = c.T
        keep = (cw > 0) & (np.abs(cx) <= cw) & (np.abs(cy) <= cw) & (np.abs(cz) <= cw)
        keep &= np.isfinite(cx / cw) & np.isfinite(cy / cw) & np.isfinite(cz / cw)
        cx, cy, cz, cw = (np.where(keep, v, 1.0) for v in (cx, cy, cz, cw))
        xw = (cx / cw * 0.5 + 0.5) * width
        yw = (cy / cw * 0.5 + 0.5) * height
        zw = cz / cw * 0.5 + 0.5
    depth = np.minimum(np.floor(zw * DEPTH_MAX + 0.5), DEPTH_MAX).astype(np.uint32)
    r = np.asarray(red, f32).reshape(-1).astype(np.float64)
    colour = np.floor(np.fmin(np.fmax(r, 0.0), 1.0) * 255.0 + 0.5).astype(np.uint32)
    x0, y0 = _gl_square_first_pixel(xw, size), _gl_square_first_pixel(yw, size)
    z0 = np.zeros(n, np.int64)
    return (keep, np.where(keep, x0, z0), np.where(keep, y0, z0), np.where(keep, depth, np.uint32(0)).astype(np.uint32),
            np.where(keep, colour, np.uint32(0)).astype(np.uint32))


def _gl_square_first_pixel(v, size):
    """The model's anchor, stated as OpenGL 3.3 section 3.4.1 states it (not through sprite_origin): the square's centre is
    floor(v) + 1/2 for odd sizes and floor(v + 1/2) for even sizes, and the square covers the pixels whose centres i + 1/2 lie
    in [centre - size/2, centre + size/2).  -> the first such pixel, ceil(centre - size/2 - 1/2), float64 throughout."""
    v = np.asarray(v, np.float64)
    centre = np.floor(v) + 0.5 if size & 1 else np.floor(v + 0.5)
    return np.ceil(centre - size / 2 - 0.5).astype(np.int64)


def scatter_min(keep, x0, y0, depth, colour, width, height, size):
    """The depth test: every pixel keeps the smallest key depth << 8 | colour over the size x size sprites covering it.
    -> uint32 [H * W] keys, EMPTY where no sprite reached."""
    frag = (depth.astype(np.uint32) << np.uint32(8)) | colour.astype(np.uint32)
    x0, y0, frag = x0[keep], y0[keep], frag[keep]
    zbuf = np.full(width * height, EMPTY, np.uint32)
    for dy in range(size):
        for dx in range(size):
            px, py = x0 + dx, y0 + dy
            ok = (px >= 0) & (px < width) & (py >= 0) & (py < height)
            np.minimum.at(zbuf, (py[ok] * width + px[ok]), frag[ok])
    return zbuf


def render_keys(xyz, red, mvp_colmajor, width, height, point_size, model=point_fragments):
    size = point_size_rule(point_size)
    return scatter_min(*model(xyz, red, mvp_colmajor, width, height, size), width, height, size)


def render_points(xyz, red, mvp_colmajor, width, height, point_size, model=point_fragments):
    """One view.  mvp_colmajor: float32[16], glm layout m[c*4+r].  Returns uint8 [H, W], bottom-up rows."""
    keys = render_keys(xyz, red, mvp_colmajor, width, height, point_size, model)
    return (keys & np.uint32(0xFF)).astype(np.uint8).reshape(height, width)


def coverage(xyz, red, mvp_colmajor, width, height, point_size, model=point_fragments):
    """One view's coverage as nmi_render_points_masked writes it: 1 where the pixel's key is not EMPTY."""
    keys = render_keys(xyz, red, mvp_colmajor, width, height, point_size, model)
    return (keys != EMPTY).astype(np.uint8).reshape(height, width)


def render_stack(xyz, red, mvps, width, height, point_size):
    return np.stack([render_points(xyz, red, m, width, height, point_size) for m in np.asarray(mvps, f32).reshape(-1, 16)])
