"""Hard homographies for the warp producer, and a numpy restatement of its per-block staging decision -- TEST INFRASTRUCTURE ONLY.

families(W, H) -> {name: [forward 3x3 float64, ...]}: the matrices each family is made of for a W x H frame.
staging_branches(M, W, H) -> how many blocks of warp_lds_block (csrc/nmi_warp_device.h) take each of its four branches.
EXPECTED_BRANCHES: the branches a family exists to reach (on frames of at least 640 x 376); a family that quietly stops
reaching them makes its tests fail instead of passing vacuously.
"""
import numpy as np

from oracle.warp_oracle_np import device_coeffs
from orbslam2_nmi_amd import synthetic as sy

f32 = np.float32

PATCH_BYTES = 16 * 1024 - 64   # kWarpPatchBytes
BLOCK_W, BLOCK_H = 128, 32     # output pixels of one warp block (32 lanes x 4 pixels, 8 rows x kWarpRowsPerThread)
BRANCHES = ("staged", "nothing", "over", "bad")


def _rot(yaw=0.0, pitch=0.0, roll=0.0):
    """R = Rz(roll) Ry(yaw) Rx(pitch), degrees."""
    a, b, c = np.radians([pitch, yaw, roll])
    Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    Rz = np.array([[np.cos(c), -np.sin(c), 0], [np.sin(c), np.cos(c), 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def rotation(W, H, **angles):
    K = sy.intrinsics(W, H)
    return K @ _rot(**angles) @ np.linalg.inv(K)


def shift(tx, ty):
    """Forward map x -> x + t: the warp samples the frame at (x - tx, y - ty)."""
    return np.array([[1.0, 0, tx], [0, 1.0, ty], [0, 0, 1.0]])


def zoom(W, H, s):
    """Forward zoom by s about a point near the frame centre: the source of pixel x is cx + (x - cx) / s.  (Not the exact
    centre: its dyadic offsets would put whole regions of the warp exactly on rounding ties.)"""
    cx, cy = 0.47 * W + 0.113, 0.53 * H - 0.071
    return np.array([[s, 0, cx * (1 - s)], [0, s, cy * (1 - s)], [0, 0, 1.0]])


def _budget_zooms(W, H):
    """Two zoom-outs about the frame centre: the largest staged patch of the first lies just under PATCH_BYTES, the second
    puts a block just over it (searched, not guessed: the box depends on floor() of the corners and on 16-byte alignment)."""
    lo, hi = 1.0, 0.2   # zoom 1: ~1.5 KiB patches; zoom 0.2: every interior block over budget
    for _ in range(40):
        mid = 0.5 * (lo + hi)
        if staging_branches(zoom(W, H, mid), W, H)["over"]:
            hi = mid
        else:
            lo = mid
    return [zoom(W, H, lo), zoom(W, H, hi)]


SCALES_POW2 = (-140, -100, -60, 60, 100, 140)
SCALES_EXTREME = (1e-38, 1e-30, 1e30, 1e39, 1e-110, 1e110)


def scale_bases(W, H):
    """The matrices the "pow2" and "extreme" families scale: a mild grid rotation (all three angles nonzero) and a 70-degree
    yaw with the horizon in view."""
    return [sy.warp_homographies(sy.intrinsics(W, H), (3, 3, 3), (0.02, 0.02, 0.05))[0], rotation(W, H, yaw=70)]


def families(W, H):
    grid = sy.warp_homographies(sy.intrinsics(W, H), (3, 3, 3), (0.02, 0.02, 0.05))
    base, steep = scale_bases(W, H)
    fam = {
        "grid": list(grid[::2]),
        # 40..70 degrees through K: the horizon (den = 0) crosses the frame for the larger angles
        "horizon": [rotation(W, H, yaw=a) for a in (40, 55, 70)] + [rotation(W, H, pitch=a) for a in (40, 55, 70)]
                   + [rotation(W, H, yaw=-62, pitch=48)],
        # 180 degrees about a point near the centre (not the principal point: where 2 cx is a dyadic fraction, whole regions
        # of the warp sit exactly on rounding ties)
        "roll180": [np.array([[-1.0, 0, W + 0.274], [0, -1, H - 0.186], [0, 0, 1]])],
        "mirror": [np.array([[-1.0, 0, W - 1], [0, 1, 0], [0, 0, 1]]), np.array([[1.0, 0, 0], [0, -1, H - 1], [0, 0, 1]])],
        "zoom": [zoom(W, H, 4.0), zoom(W, H, 0.25)],
        "budget": _budget_zooms(W, H),
        # integer and half-pixel shifts; |t| <= 2 puts source columns exactly on -2, -1, W - 1, W and W + 1; t = +-(W + 1)
        # puts one column exactly on the far bound
        "shift": [shift(t, 0) for t in (1, -1, 2, -2, 0.5, -0.5, W + 1, -(W + 1))]
                 + [shift(0, t) for t in (1, -2, 2, -0.5, H + 1)] + [shift(3, -5), shift(-1.5, 2.5)],
        "out_of_frame": [shift(3 * W + 40, 3 * H + 40), shift(-3 * W - 40, 0.5)],
        "one_axis": [shift(0, 3 * H + 40), shift(-3 * W - 40, 0)],
        # pow2[i * len(SCALES_POW2) + j] = 2^SCALES_POW2[j] scale_bases[i]; extreme likewise with SCALES_EXTREME
        "pow2": [np.ldexp(M, k) for M in (base, steep) for k in SCALES_POW2],
        "extreme": [s * M for M in (base, steep) for s in SCALES_EXTREME],
    }
    return fam


EXPECTED_BRANCHES = {
    "grid": {"staged"},
    "horizon": {"bad", "staged"},
    "roll180": {"staged"},
    "mirror": {"staged"},
    "zoom": {"staged", "over"},
    "budget": {"staged", "over"},
    "shift": {"staged"},
    "out_of_frame": {"nothing"},
    "one_axis": {"nothing"},
    "pow2": {"staged", "bad"},
    "extreme": {"staged", "bad"},
}


def staging_branches(M, W, H, sizes=False):
    """Per-block decision of warp_lds_block restated: the four block corners through the kernel's fp32 expressions (with the
    product's coefficients), the box grown by 2 pixels and clipped to [-2, W + 1] x [-2, H + 1], pitch * rows against the
    LDS budget, and the all_good test (den > 0, |xs|, |ys| < 1e8 at every corner).  -> {branch: number of blocks}, plus
    "max_staged" (the largest staged patch, bytes) when sizes=True."""
    c = device_coeffs(M)
    nbx = ((W + 3) // 4 + 31) // 32
    nby = (H + BLOCK_H - 1) // BLOCK_H
    bx0 = np.arange(nbx) * BLOCK_W
    by0 = np.arange(nby) * BLOCK_H
    bx1, by1 = np.minimum(bx0 + BLOCK_W - 1, W - 1), np.minimum(by0 + BLOCK_H - 1, H - 1)
    X = np.stack(np.broadcast_arrays(bx0[None, :], bx1[None, :], bx0[None, :], bx1[None, :]), -1).astype(f32)
    Y = np.stack(np.broadcast_arrays(by0[:, None], by0[:, None], by1[:, None], by1[:, None]), -1).astype(f32)
    X, Y = np.broadcast_to(X, (nby, nbx, 4)), np.broadcast_to(Y, (nby, nbx, 4))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        den = (c[6] * X + c[7] * Y) + c[8]
        coeff = f32(1.0) / den
        xs = coeff * ((c[0] * X + c[1] * Y) + c[2])
        ys = coeff * ((c[3] * X + c[4] * Y) + c[5])
        good = ((den > 0) & (np.abs(xs) < f32(1e8)) & (np.abs(ys) < f32(1e8))).all(-1)
    out = dict.fromkeys(BRANCHES, 0)
    max_staged = 0
    for j in range(nby):
        for i in range(nbx):
            if not good[j, i]:
                out["bad"] += 1
                continue
            x_lo = max(int(np.floor(xs[j, i].min())) - 2, -2)
            x_hi = min(int(np.floor(xs[j, i].max())) + 3, W + 1)
            y_lo = max(int(np.floor(ys[j, i].min())) - 2, -2)
            y_hi = min(int(np.floor(ys[j, i].max())) + 3, H + 1)
            if x_lo > x_hi or y_lo > y_hi:
                out["nothing"] += 1
                continue
            px0 = -16 if x_lo < 0 else x_lo & ~15
            nbytes = (((x_hi - px0 + 1) + 15) & ~15) * (y_hi - y_lo + 1)
            if nbytes > PATCH_BYTES:
                out["over"] += 1
            else:
                out["staged"] += 1
                max_staged = max(max_staged, nbytes)
    if sizes:
        out["max_staged"] = max_staged
    return out


def branches_reached(Ms, W, H):
    """Names of the branches that at least one block of one of the matrices takes."""
    seen = set()
    for M in Ms:
        seen |= {b for b, n in staging_branches(M, W, H).items() if n}
    return seen
