"""numpy restatement of the lens undistortion (nmi_undistort_frame, include/nmi_hip.h) -- TEST INFRASTRUCTURE ONLY.

twin: the product's fp32 arithmetic in the order the header states it (numpy float32 rounds every operation, the kernel is
built with -ffp-contract=off), the bilinear value of the warp kernels (oracle/warp_oracle_np.py) and the validity rule of the
warp masks (helpers/masked_np.py) at the resulting source coordinate -- byte for byte.
float64 model: the same map and value in double, for the tie-distance criterion of tests/test_warp_edges.py.
distort_image: the forward direction in double (a pinhole image seen through the lens), to make a camera frame from a
render for the recovery test.
"""
import numpy as np

f32 = np.float32

# Coefficient families (k1, k2, p1, p2, k3) for a camera of the ETH / synthetic.intrinsics kind (fx ~ 0.7 W).
FAMILIES = {
    "barrel": (-0.28, 0.074, 0.0, 0.0, 0.0),         # a wide-angle MAV camera
    "pincushion": (0.18, 0.03, 0.0, 0.0, 0.0),
    "tangential": (0.0, 0.0, 0.0021, -0.0017, 0.0),
    "strong_k3": (-0.31, 0.12, 0.0009, 0.0004, -0.06),
    "folded": (-0.9, 0.0, 0.0, 0.0, 0.0),             # 1 + k1 r^2 changes sign inside the frame: the map folds over
}


def params(K, dist):
    """-> dict of the fp32 constants the host hands to the kernel."""
    K = np.asarray(K, np.float64).reshape(9)
    d = np.asarray(dist, f32).reshape(5)
    return dict(fx=f32(K[0]), fy=f32(K[4]), cx=f32(K[2]), cy=f32(K[5]), ifx=f32(1.0 / K[0]), ify=f32(1.0 / K[4]),
                k1=d[0], k2=d[1], p1=d[2], p2=d[3], k3=d[4])


def source_coords(shape, K, dist):
    """-> fp32 (xs, ys) [H, W]: where output pixel (u, v) samples the raw frame, as the kernel computes it."""
    h, w = shape
    p = params(K, dist)
    vv, uu = np.mgrid[0:h, 0:w]
    u, v = uu.astype(f32), vv.astype(f32)
    with np.errstate(over="ignore", invalid="ignore"):
        x = (u - p["cx"]) * p["ifx"]
        y = (v - p["cy"]) * p["ify"]
        x2, y2, xy = x * x, y * y, x * y
        r2 = x2 + y2
        rad = r2 * (p["k1"] + r2 * (p["k2"] + r2 * p["k3"]))
        two = f32(2)
        dx = ((x * rad) + ((two * p["p1"]) * xy)) + (p["p2"] * (r2 + two * x2))
        dy = ((y * rad) + (p["p1"] * (r2 + two * y2))) + ((two * p["p2"]) * xy)
        xs = u + p["fx"] * dx
        ys = v + p["fy"] * dy
    assert xs.dtype == f32 and ys.dtype == f32
    return xs, ys


def sample(img, xs, ys):
    """warp_sample_global in numpy: reach test, bilinear taps with a zero border, round half even, clamp."""
    h, w = img.shape
    with np.errstate(invalid="ignore"):
        inside = (xs > f32(-2)) & (xs < f32(w + 1)) & (ys > f32(-2)) & (ys < f32(h + 1))
    xs = np.where(inside, xs, f32(-10))
    ys = np.where(inside, ys, f32(-10))
    x1 = np.floor(xs).astype(np.int64)
    y1 = np.floor(ys).astype(np.int64)
    x2, y2 = x1 + 1, y1 + 1

    def tap(yi, xi):
        ok = (xi >= 0) & (xi < w) & (yi >= 0) & (yi < h)
        return np.where(ok, img[np.clip(yi, 0, h - 1), np.clip(xi, 0, w - 1)], 0).astype(f32)

    ax2, ax1 = x2.astype(f32) - xs, xs - x1.astype(f32)
    ay2, ay1 = y2.astype(f32) - ys, ys - y1.astype(f32)
    acc = np.zeros(xs.shape, f32)
    acc = acc + tap(y1, x1) * (ax2 * ay2)
    acc = acc + tap(y1, x2) * (ax1 * ay2)
    acc = acc + tap(y2, x1) * (ax2 * ay1)
    acc = acc + tap(y2, x2) * (ax1 * ay1)
    return np.clip(np.rint(acc), 0, 255).astype(np.uint8)


def valid(shape, xs, ys, mask=None):
    """warp_source_valid in numpy: the reach test, every tap with nonzero weight inside the frame (and nonzero in mask)."""
    h, w = shape
    with np.errstate(invalid="ignore"):
        inside = (xs > f32(-2)) & (xs < f32(w + 1)) & (ys > f32(-2)) & (ys < f32(h + 1))
    xs = np.where(inside, xs, f32(0))
    ys = np.where(inside, ys, f32(0))
    x1 = np.floor(xs).astype(np.int64)
    y1 = np.floor(ys).astype(np.int64)
    x2 = x1 + (xs != x1.astype(f32))
    y2 = y1 + (ys != y1.astype(f32))
    ok = inside & (x1 >= 0) & (y1 >= 0) & (x2 <= w - 1) & (y2 <= h - 1)
    if mask is not None:
        m = np.asarray(mask) != 0
        cx1, cx2 = np.clip(x1, 0, w - 1), np.clip(x2, 0, w - 1)
        cy1, cy2 = np.clip(y1, 0, h - 1), np.clip(y2, 0, h - 1)
        ok &= m[cy1, cx1] & m[cy1, cx2] & m[cy2, cx1] & m[cy2, cx2]
    return ok.astype(np.uint8)


def undistort(raw, K, dist, raw_mask=None):
    """-> (frame [H, W] u8, mask [H, W] u8): the product's bytes."""
    raw = np.asarray(raw, np.uint8)
    xs, ys = source_coords(raw.shape, K, dist)
    return sample(raw, xs, ys), valid(raw.shape, xs, ys, raw_mask)


# ------------------------------------------------------------------------------------------------------------ float64

def source_coords_f64(shape, K, dist):
    """-> float64 (u_d, v_d): the textbook u_d = fx x_d + cx of the same map."""
    h, w = shape
    K = np.asarray(K, np.float64).reshape(9)
    k1, k2, p1, p2, k3 = (float(v) for v in np.asarray(dist, f32))
    vv, uu = np.mgrid[0:h, 0:w].astype(np.float64)
    x, y = (uu - K[2]) / K[0], (vv - K[5]) / K[4]
    r2 = x * x + y * y
    rad = 1 + r2 * (k1 + r2 * (k2 + r2 * k3))
    xd = x * rad + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
    yd = y * rad + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
    return K[0] * xd + K[2], K[4] * yd + K[5]


def bilinear_f64(img, u, v):
    """float64 bilinear value at (u, v) with a zero border; 0 where the source is out of reach (as the product's test)."""
    h, w = img.shape
    reach = (u > -2) & (u < w + 1) & (v > -2) & (v < h + 1)
    u, v = np.where(reach, u, -10.0), np.where(reach, v, -10.0)
    x0, y0 = np.floor(u).astype(np.int64), np.floor(v).astype(np.int64)
    fx, fy = u - x0, v - y0
    src = np.pad(img.astype(np.float64), 1)

    def at(yi, xi):
        ok = (xi >= -1) & (xi <= w) & (yi >= -1) & (yi <= h)
        return np.where(ok, src[np.clip(yi, -1, h) + 1, np.clip(xi, -1, w) + 1], 0.0)

    val = ((1 - fx) * (1 - fy) * at(y0, x0) + fx * (1 - fy) * at(y0, x0 + 1)
           + (1 - fx) * fy * at(y0 + 1, x0) + fx * fy * at(y0 + 1, x0 + 1))
    return np.where(reach, val, 0.0)


def undistort_value_f64(raw, K, dist):
    """The float64 value of every output pixel (before rounding)."""
    u, v = source_coords_f64(np.asarray(raw).shape, K, dist)
    return bilinear_f64(np.asarray(raw, np.uint8), u, v)


def distort_image(pinhole, K, dist, iters=40):
    """The camera frame a lens with these coefficients makes of a pinhole image (float64): raw pixel (ud, vd) shows the
    pinhole image at the undistorted point of (ud, vd), found by the fixed-point iteration of cv::undistortPoints."""
    h, w = pinhole.shape
    K = np.asarray(K, np.float64).reshape(9)
    k1, k2, p1, p2, k3 = (float(v) for v in dist)
    vv, uu = np.mgrid[0:h, 0:w].astype(np.float64)
    xd, yd = (uu - K[2]) / K[0], (vv - K[5]) / K[4]
    x, y = xd.copy(), yd.copy()
    for _ in range(iters):
        r2 = x * x + y * y
        rad = 1 + r2 * (k1 + r2 * (k2 + r2 * k3))
        tx = 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
        ty = p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
        x, y = (xd - tx) / rad, (yd - ty) / rad
    val = bilinear_f64(np.asarray(pinhole, np.uint8), K[0] * x + K[2], K[4] * y + K[5])
    return np.clip(np.rint(val), 0, 255).astype(np.uint8)
