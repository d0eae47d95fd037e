"""The refined-peaks rule of include/nmi_hip.h ("Refined peaks") in numpy scalars, and the tables and keys the tests refine
-- TEST INFRASTRUCTURE ONLY.

refine(table, num, keys, dtype) -> records (numpy structured array, one per key).  dtype = np.float32 is the BIT-EXACT model: every
value is a np.float32 scalar and every operation rounds once, in the order the header writes, so the records equal the device's
and the host twin's byte for byte (record_dtype(np.float32) has nmi_refined_peak's layout).  dtype = np.float64 is the ACCURACY
model: the same rule without fp32's rounding.
It shares nothing with the kernel (csrc/nmi_refine.hip) or the host twin (host/nmi_refine_host.cpp), which share their arithmetic
(host/nmi_refine_rule.h: six fixed axes with inactive ones skipped, samples by number, strides), but the rule: here the table is a
6-D array indexed by coordinates, and the active axes are compacted into a dense n x n system before the L D L^T.
Cases are built on tests/helpers/peaks_np.py: its shapes, its contents plus two quadratic ones, its ranked keys.
"""
import functools

import numpy as np

from helpers import peaks_np as pk

EMPTY, NONFINITE, COUPLED, CROSS_HOLE = 1, 2, 4, 8
MAX_K = 64


def BORDER(a):
    return 0x100 << a


def HOLE(a):
    return 0x10000 << a


def FLAT(a):
    return 0x1000000 << a


@functools.lru_cache(maxsize=None)
def record_dtype(dtype):
    f = np.dtype(dtype)
    return np.dtype([("key", np.uint64), ("offset", f, 6), ("score", f), ("flags", np.uint32), ("gradient", f, 6), ("hessian", f, 21),
                     ("reserved", np.uint32)])


assert record_dtype(np.float32).itemsize == 152


def refine(table, num, keys, dtype=np.float32):
    F = np.dtype(dtype).type
    zero, one, half, quarter = F(0), F(1), F(0.5), F(0.25)
    num = [int(v) for v in num]
    t = np.asarray(table).astype(dtype).reshape(tuple(reversed(num)))     # t[c5, c4, c3, c2, c1, c0]
    out = np.zeros(len(keys), record_dtype(dtype))

    def usable(v):
        return bool(v >= 0) and bool(np.isfinite(v))

    with np.errstate(all="ignore"):
        for r, key in zip(out, keys):
            key = int(key)
            index = 0xFFFFFFFF - (key & 0xFFFFFFFF)
            if key == 0 or index >= t.size:
                r["flags"] = EMPTY
                continue
            c = [int(v) for v in np.unravel_index(index, t.shape)][::-1]

            def at(*moves):
                cc = list(c)
                for a, d in moves:
                    cc[a] += d
                    assert 0 <= cc[a] < num[a]      # the rule never leaves the grid
                return t[tuple(reversed(cc))]

            r["key"] = key
            f0 = at()
            if not usable(f0):
                r["score"], r["flags"] = f0, NONFINITE
                continue
            flags, act = 0, []
            g, H = [zero] * 6, [[zero] * 6 for _ in range(6)]
            for a in range(6):
                if num[a] == 1:
                    continue
                if c[a] < 1 or c[a] > num[a] - 2:
                    flags |= BORDER(a)
                    continue
                fp, fm = at((a, 1)), at((a, -1))
                if not (usable(fp) and usable(fm)):
                    flags |= HOLE(a)
                    continue
                act.append(a)
                g[a] = half * (fp - fm)
                H[a][a] = (fp - f0) + (fm - f0)
            for i, a in enumerate(act):
                for b in act[i + 1:]:
                    fpp, fpm, fmp, fmm = at((a, 1), (b, 1)), at((a, 1), (b, -1)), at((a, -1), (b, 1)), at((a, -1), (b, -1))
                    if all(usable(v) for v in (fpp, fpm, fmp, fmm)):
                        H[a][b] = H[b][a] = quarter * ((fpp - fpm) - (fmp - fmm))
                    else:
                        flags |= CROSS_HOLE
            # coupled step on the dense system of the active axes
            n = len(act)
            x = None
            if n:
                A = [[-H[a][b] for b in act] for a in act]
                L, d, ok = [[zero] * n for _ in range(n)], [], True
                for j in range(n):
                    v = A[j][j]
                    for k in range(j):
                        v = v - (L[j][k] * d[k]) * L[j][k]
                    d.append(v)
                    if not v > 0:
                        ok = False
                        break
                    for i in range(j + 1, n):
                        w = A[i][j]
                        for k in range(j):
                            w = w - (L[i][k] * d[k]) * L[j][k]
                        L[i][j] = w / v
                if ok:
                    z = []
                    for i in range(n):
                        v = g[act[i]]
                        for k in range(i):
                            v = v - L[i][k] * z[k]
                        z.append(v)
                    x = [zero] * n
                    for i in reversed(range(n)):
                        v = z[i] / d[i]
                        for k in range(i + 1, n):
                            v = v - L[k][i] * x[k]
                        x[i] = v
                    if not all(bool(v >= -one) and bool(v <= one) for v in x):
                        x = None
            delta = [zero] * 6
            if x is not None:
                flags |= COUPLED
                for i, a in enumerate(act):
                    delta[a] = x[i]
            else:
                for a in act:
                    if H[a][a] < 0:
                        v = (-g[a]) / H[a][a]
                        delta[a] = -one if v < -one else one if v > one else v
                    else:
                        flags |= FLAT(a)
            lin, quad = zero, zero
            for a in act:
                lin = lin + g[a] * delta[a]
                row = zero
                for b in act:
                    row = row + H[a][b] * delta[b]
                quad = quad + delta[a] * row
            r["score"] = (f0 + lin) + half * quad
            r["flags"] = flags
            r["offset"], r["gradient"] = delta, g
            r["hessian"] = [H[a][b] for a in range(6) for b in range(a, 6)]
    return out


def hessian_matrix(record):
    """The 6 x 6 symmetric matrix of a record's upper triangle."""
    H = np.zeros((6, 6), record["hessian"].dtype)
    H[np.triu_indices(6)] = record["hessian"]
    return H + np.triu(H, 1).T


def same_bytes(got, want):
    """Every bit of every record (a NaN score compares by its bits)."""
    return np.asarray(got).tobytes() == np.asarray(want).tobytes()


def explain(got, want):
    """The first record that differs, for an assertion's message."""
    for k, (a, b) in enumerate(zip(got, want)):
        if a.tobytes() != b.tobytes():
            return f"record {k}: got {a} want {b}"
    return "equal"


# ---- the case list ---------------------------------------------------------------------------------------------------------------
SHAPES = pk.SHAPES                                       # the host twin's; the 65,536-cell shape included
GPU_SHAPES = [(1, 1, 1, 1, 1, 1), (3, 1, 1, 1, 1, 1), (3, 3, 3, 3, 3, 3), (3, 3, 3, 3, 3, 1), (1, 3, 3, 3, 3, 3), (5, 13, 1, 1, 1, 1),
              (16, 16, 16, 4, 2, 2)]
ABOVE_PEAKS_LIMIT = pk.TOO_LARGE                         # 65,537 cells: no limit here
CONTENTS = pk.CONTENTS + ("bowl", "ridge")
RADII = [(0,) * 6, (1,) * 6]
KS = (1, 2, 64)


def table(num, content):
    """float32 [cells] of the case: peaks_np's contents, and two quadratics -- "bowl" (one smooth nonnegative maximum between the
    cells near the grid's middle, so that every interior axis is active and the step is coupled) and "ridge" (the same with strongly
    coupled axes at the size of real NMI tables, 0.08, under noise of a tenth of its curvature)."""
    if content in pk.CONTENTS:
        return pk.table(num, content)
    rng = np.random.default_rng([17, *num, CONTENTS.index(content)])
    at = pk.coordinates(num).astype(np.float64)
    centre = (np.asarray(num, np.float64) - 1) / 2 + rng.uniform(-0.4, 0.4, 6)
    M = rng.standard_normal((6, 6))
    if content == "bowl":
        c0, A = 0.9, 0.01 * (M @ M.T / 6 + np.eye(6))
    else:
        M[:, 0] *= 3
        c0, A = 0.08, 0.002 * (M @ M.T / 6 + np.eye(6))
    d = at - centre[:, None]
    t = c0 - np.einsum("an,ab,bn->n", d, A, d)
    if content == "ridge":
        t += rng.uniform(-2e-4, 2e-4, t.size)
    return t.astype(np.float32)


@functools.lru_cache(maxsize=None)
def keys_of(num, content, radius):
    """The MAX_K ranked keys of the case (peaks_np's model; zeros after the peaks)."""
    if content in pk.CONTENTS:
        return pk.ranked(num, content, radius)[0]
    return pk.find_peaks(table(num, content), num, MAX_K, radius)[0]


@functools.lru_cache(maxsize=None)
def refined(num, content, radius):
    """The float32 model's MAX_K records of the case: record k depends on key k alone, so callers take prefixes (and do not write
    into it)."""
    return refine(table(num, content), num, keys_of(num, content, radius), np.float32)


# ---- accuracy: planted quadratics --------------------------------------------------------------------------------------------
NUM3 = (3, 3, 3, 3, 3, 3)
CENTRE_KEY_INDEX = 364                                   # the cell (1, 1, 1, 1, 1, 1) of 3^6
MAGNITUDES = {"large": (0.9, 0.01), "nmi": (0.08, 0.002)}   # c0, the scale of A = scale * (M M^T / 6 + I)
CPU_SEEDS, GPU_SEEDS = (1, 2), (3, 4)                    # 100 cases a seed: 200 on the CPU tier, 200 unseen on the GPU tier
CASES_PER_SEED = 100
# The float32 model against the float64 model on the same float32 table, largest deviation over the kept cases of CPU_SEEDS, as
# tests/test_refine_model.py::test_accuracy measures (and prints) them:
#   offset  8.047e-8 cells at "large" (197 of 200 kept), 7.376e-8 at "nmi" (193 of 200 kept)
#   score   4.532e-8 at "large", 5.680e-9 at "nmi"
# (small because the rule's differences of neighbouring samples are exact in fp32: what rounds is the solve.)  The larger of each
# rounded up to three digits (8.05e-8, 4.54e-8) is the constant; both tiers allow 4 x that, which is there for the two unseen seeds of the GPU tier.
MEASURED_OFFSET, MEASURED_SCORE = 8.05e-8, 4.54e-8
OFFSET_TOLERANCE, SCORE_TOLERANCE = 4 * MEASURED_OFFSET, 4 * MEASURED_SCORE


def planted(seed, magnitude):
    """-> [(table float64 [729], planted offset float64 [6], A)] : c0 - (x - x*)^T A (x - x*) on 3^6 with x* = the centre cell + an
    offset uniform in +-0.35."""
    c0, scale = MAGNITUDES[magnitude]
    rng = np.random.default_rng([seed, sorted(MAGNITUDES).index(magnitude)])
    at = pk.coordinates(NUM3).astype(np.float64)
    out = []
    for _ in range(CASES_PER_SEED):
        M = rng.standard_normal((6, 6))
        A = scale * (M @ M.T / 6 + np.eye(6))
        offset = rng.uniform(-0.35, 0.35, 6)
        d = at - (1.0 + offset)[:, None]
        out.append((c0 - np.einsum("an,ab,bn->n", d, A, d), offset, A))
    return out


def centre_key(t):
    """The key of the centre cell of a 3^6 table (the score bits are not used by the rule; they are the cell's own)."""
    return pk.keys_of(t)[CENTRE_KEY_INDEX]


def kept(t64):
    """-> (t32, model64 record on t32) when the case counts, else None: the centre is the arg-max, the table is nonnegative, and
    the float64 model takes the coupled step, on the float64 and on the float32 table, with |offset| <= 0.45."""
    t32 = t64.astype(np.float32)
    if int(t64.argmax()) != CENTRE_KEY_INDEX or int(t32.argmax()) != CENTRE_KEY_INDEX or t64.min() < 0:
        return None
    key = [centre_key(t32)]
    exact, m64 = refine(t64, NUM3, key, np.float64)[0], refine(t32, NUM3, key, np.float64)[0]
    for r in (exact, m64):
        if not r["flags"] & COUPLED or np.abs(r["offset"]).max() > 0.45:
            return None
    return t32, m64
