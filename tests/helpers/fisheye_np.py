"""numpy restatement of the fisheye undistortion (nmi_undistort_frame_fisheye, include/nmi_hip.h) -- TEST INFRASTRUCTURE ONLY.

twin: the product's fp32 arithmetic in the order the header states it (numpy float32 rounds every operation, np.sqrt and the
division are correctly rounded as the kernel's are, and the arctangent is the header's spelled-out one, not np.arctan), then
the value and validity rules of helpers/undistort_np.py at the resulting source coordinate -- byte for byte.
float64 model: the textbook map (np.arctan) and value in double, for the tie-distance criterion of tests/test_warp_edges.py.
fisheye_image: the forward direction in double (a pinhole image seen through the lens), to make a camera frame from a render
for the recovery test.
"""
import numpy as np

from helpers import undistort_np as unp

f32 = np.float32

# Coefficient families (k1, k2, k3, k4) of the equidistant model.
FAMILIES = {
    "zero": (0.0, 0.0, 0.0, 0.0),                          # an ideal equidistant lens: still a remap
    "tumvi": (0.00348, 0.000715, -0.00205, 0.000203),      # a TUM-VI camera
    "euroc_eq": (-0.01372, -0.02073, 0.03443, -0.01995),   # an equidistant calibration of a EuRoC camera
    "strong": (-0.12, 0.03, -0.008, 0.001),
    "folded": (-1.2, 0.0, 0.0, 0.0),                       # theta (1 + k1 theta^2) turns back inside the frame
}
REGULAR = [f for f in FAMILIES if f != "folded"]
FOCAL_SCALES = (1.0, 0.5, 0.35)


def raw_K(W, H):
    """The raw camera: focal lengths about 0.45 W (a lens of some 96 degrees across), the principal point off the centre."""
    return np.array([[0.45 * W, 0, 0.5 * W - 0.5 + 0.021 * W], [0, 0.4525 * W, 0.5 * H - 0.5 - 0.017 * H], [0, 0, 1.0]])


def pinhole_K(K_raw, scale):
    """The output camera: K_raw with the focal lengths multiplied by scale (below 1: a wider pinhole view)."""
    K = np.array(K_raw, np.float64).reshape(3, 3).copy()
    K[0, 0] *= scale
    K[1, 1] *= scale
    return K


def params(K, K_raw, dist):
    """-> dict of the fp32 constants the host hands to the kernel."""
    K = np.asarray(K, np.float64).reshape(9)
    R = K if K_raw is None else np.asarray(K_raw, np.float64).reshape(9)
    d = np.asarray(dist, f32).reshape(4)
    return dict(cxn=f32(K[2]), cyn=f32(K[5]), ifx=f32(1.0 / K[0]), ify=f32(1.0 / K[4]), fx=f32(R[0]), fy=f32(R[4]), cx=f32(R[2]),
                cy=f32(R[5]), k1=d[0], k2=d[1], k3=d[2], k4=d[3])


def atan32(r):
    """The header's arctangent of r >= 0, in float32 operations."""
    one = f32(1)
    big = r > f32(2.414213562373095)
    mid = ~big & (r > f32(0.4142135623730950))
    with np.errstate(divide="ignore", invalid="ignore"):
        a = np.where(big, -one / r, np.where(mid, (r - one) / (r + one), r)).astype(f32)
    base = np.where(big, f32(np.pi / 2), np.where(mid, f32(np.pi / 4), f32(0))).astype(f32)
    z = a * a
    q = ((f32(8.05374449538e-2) * z - f32(1.38776856032e-1)) * z + f32(1.99777106478e-1)) * z - f32(3.33329491539e-1)
    theta = base + ((q * z) * a + a)
    assert theta.dtype == f32
    return theta


def source_coords(shape, K, K_raw, dist):
    """-> fp32 (xs, ys) [H, W]: where output pixel (u, v) samples the raw frame, as the kernel computes it."""
    h, w = shape
    p = params(K, K_raw, dist)
    vv, uu = np.mgrid[0:h, 0:w]
    u, v = uu.astype(f32), vv.astype(f32)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        x = (u - p["cxn"]) * p["ifx"]
        y = (v - p["cyn"]) * p["ify"]
        r2 = x * x + y * y
        r = np.sqrt(r2)
        theta = atan32(r)
        t2 = theta * theta
        td = theta + theta * (t2 * (p["k1"] + t2 * (p["k2"] + t2 * (p["k3"] + t2 * p["k4"]))))
        s = np.where(r > f32(1e-8), td / r, f32(1)).astype(f32)
        xs = p["cx"] + p["fx"] * (x * s)
        ys = p["cy"] + p["fy"] * (y * s)
    assert xs.dtype == f32 and ys.dtype == f32
    return xs, ys


def undistort(raw, K, K_raw, dist, raw_mask=None):
    """-> (frame [H, W] u8, mask [H, W] u8): the product's bytes."""
    raw = np.asarray(raw, np.uint8)
    xs, ys = source_coords(raw.shape, K, K_raw, dist)
    return unp.sample(raw, xs, ys), unp.valid(raw.shape, xs, ys, raw_mask)


# ------------------------------------------------------------------------------------------------------------ float64

def theta_d(theta, dist):
    k1, k2, k3, k4 = (float(v) for v in np.asarray(dist, f32))
    t2 = theta * theta
    return theta * (1 + t2 * (k1 + t2 * (k2 + t2 * (k3 + t2 * k4))))


def source_coords_f64(shape, K, K_raw, dist):
    """-> float64 (u_d, v_d): the textbook form of the same map."""
    h, w = shape
    K = np.asarray(K, np.float64).reshape(9)
    R = K if K_raw is None else np.asarray(K_raw, np.float64).reshape(9)
    vv, uu = np.mgrid[0:h, 0:w].astype(np.float64)
    x, y = (uu - K[2]) / K[0], (vv - K[5]) / K[4]
    r = np.hypot(x, y)
    td = theta_d(np.arctan(r), dist)
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.where(r > 0, td / r, 1.0)
    return R[0] * (x * s) + R[2], R[4] * (y * s) + R[5]


def undistort_value_f64(raw, K, K_raw, dist):
    """The float64 value of every output pixel (before rounding)."""
    u, v = source_coords_f64(np.asarray(raw).shape, K, K_raw, dist)
    return unp.bilinear_f64(np.asarray(raw, np.uint8), u, v)


def fisheye_image(pinhole, K, K_raw, dist, iters=30):
    """The raw frame a fisheye camera (K_raw, dist) makes of a pinhole image taken with K (float64): a raw pixel gives its
    normalised distorted point, Newton solves td(theta) = |point| from theta = |point|, r = tan(theta) puts the ray on the
    pinhole's plane, and the pinhole image is read there bilinearly.  Rays at 90 degrees or more show nothing (0)."""
    h, w = pinhole.shape
    K = np.asarray(K, np.float64).reshape(9)
    R = K if K_raw is None else np.asarray(K_raw, np.float64).reshape(9)
    k1, k2, k3, k4 = (float(v) for v in np.asarray(dist, f32))
    vv, uu = np.mgrid[0:h, 0:w].astype(np.float64)
    xd, yd = (uu - R[2]) / R[0], (vv - R[5]) / R[4]
    rd = np.hypot(xd, yd)
    theta = rd.copy()
    for _ in range(iters):
        t2 = theta * theta
        f = theta * (1 + t2 * (k1 + t2 * (k2 + t2 * (k3 + t2 * k4)))) - rd
        df = 1 + t2 * (3 * k1 + t2 * (5 * k2 + t2 * (7 * k3 + t2 * 9 * k4)))
        theta = theta - f / df
    seen = (theta >= 0) & (theta < np.pi / 2 - 1e-6)
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.where(rd > 0, np.tan(np.where(seen, theta, 0.0)) / rd, 1.0)
    u = np.where(seen, K[0] * (xd * s) + K[2], -10.0)
    v = np.where(seen, K[4] * (yd * s) + K[5], -10.0)
    return np.clip(np.rint(unp.bilinear_f64(np.asarray(pinhole, np.uint8), u, v)), 0, 255).astype(np.uint8)


class FisheyeCtx:
    """A context whose undistort_frame(raw, K, dist, ...) is undistort_frame_fisheye(raw, K, K_raw, dist, ...), everything else
    the context's own: the chain harnesses of tests/test_undistort_level.py, test_color_level.py and test_reduce_level.py then
    compute the fisheye chain unchanged."""

    def __init__(self, ctx, K_raw):
        self._ctx, self._K_raw = ctx, K_raw

    def undistort_frame(self, raw, K, dist, **kw):
        return self._ctx.undistort_frame_fisheye(raw, K, self._K_raw, dist, **kw)

    def __getattr__(self, name):
        return getattr(self._ctx, name)
