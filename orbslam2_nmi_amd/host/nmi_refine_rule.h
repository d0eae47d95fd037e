// nmi_refine_rule.h -- internal: the refined-peaks rule of include/nmi_hip.h ("Refined peaks"), written once for the kernel
// (csrc/nmi_refine.hip) and for the host twin (host/nmi_refine_host.cpp).  Plain fp32 + - * / in a fixed order, one rounding per
// operation: both sides are compiled without contraction and without fast-math, so both give the same bits -- those of the numpy
// model of tests/helpers/refine_np.py, which is the executable statement of the rule.
//
// Two pieces: refine_sample_cell says which cell of the table sample s of a record is (the gather), refine_rule turns the 73
// gathered samples into the record (everything after the gather).  Every loop has constant bounds and is unrolled, and every array
// is indexed by constants after unrolling, so that the kernel keeps them in registers.
#pragma once
#include <stdint.h>

#include "nmi_refined_peak.h"

#if defined(__HIPCC__)
#define NMI_REFINE_HD __host__ __device__ inline
#else
#define NMI_REFINE_HD inline
#endif
#if defined(__clang__)
#define NMI_REFINE_UNROLL _Pragma("unroll")
#elif defined(__GNUC__)
#define NMI_REFINE_UNROLL _Pragma("GCC unroll 6")
#else
#define NMI_REFINE_UNROLL
#endif

namespace nmi {

constexpr int kRefineMaxK = 64;      // records per call
constexpr int kRefineSamples = 73;   // the centre, 6 x 2 axial neighbours, 15 x 4 corners
constexpr int kRefineWords = 38;     // 32-bit words of a record

static_assert(sizeof(nmi_refined_peak) == 4 * kRefineWords, "nmi_refined_peak is 152 bytes");

// Sample numbering.  0: the centre.  1 + 2 a + m: the axial neighbour of axis a, m = 0 at +1, m = 1 at -1.
// 13 + 4 p + q: corner q of pair p; the pairs a < b are numbered (0,1) (0,2) .. (0,5) (1,2) .. (4,5), the corners
// q = 0 (+,+), 1 (+,-), 2 (-,+), 3 (-,-) as (step on a, step on b).
// -> the linear index of the cell of sample s around the cell `centre` with coordinates c; a sample that would leave the grid on one
// of its axes is the centre again (its value is then never used: that axis is a border axis).
NMI_REFINE_HD uint32_t refine_sample_cell(int s, uint32_t centre, const int32_t c[6], const int32_t num[6], const uint32_t stride[6])
{
    int a = -1, b = -1, da = 0, db = 0;
    if (s >= 13) {
        const int p = (s - 13) >> 2, q = (s - 13) & 3;
        int at = 0;
        NMI_REFINE_UNROLL
        for (int i = 0; i < 6; ++i) {
            NMI_REFINE_UNROLL
            for (int j = i + 1; j < 6; ++j) {
                if (at == p) a = i, b = j;
                ++at;
            }
        }
        da = (q & 2) ? -1 : 1;
        db = (q & 1) ? -1 : 1;
    } else if (s >= 1) {
        a = (s - 1) >> 1;
        da = ((s - 1) & 1) ? -1 : 1;
    }
    int64_t cell = (int64_t)centre;
    bool inside = true;
    NMI_REFINE_UNROLL
    for (int i = 0; i < 6; ++i) {
        const int d = i == a ? da : i == b ? db : 0;
        const int32_t at = c[i] + d;
        if (at < 0 || at >= num[i]) inside = false;
        cell += (int64_t)d * (int64_t)stride[i];
    }
    return inside ? (uint32_t)cell : centre;
}

// >= 0 (so -0.0 is) and finite
NMI_REFINE_HD bool refine_usable(float v) { return v >= 0.0f && v <= 3.402823466e+38f; }

// The record of the peak at coordinates c with key `key` from its samples f[kRefineSamples] (numbered as above).
NMI_REFINE_HD void refine_rule(const float *f, const int32_t c[6], const int32_t num[6], uint64_t key, nmi_refined_peak *r)
{
    uint32_t flags = 0;
    bool act[6];
    float g[6], H[6][6], x[6];
    NMI_REFINE_UNROLL
    for (int a = 0; a < 6; ++a) {
        act[a] = false;
        g[a] = 0.0f;
        x[a] = 0.0f;
        NMI_REFINE_UNROLL
        for (int b = 0; b < 6; ++b) H[a][b] = 0.0f;
    }
    const float f0 = f[0];
    float score = f0;
    if (!refine_usable(f0)) {
        flags = NMI_REFINE_NONFINITE;
    } else {
        // active axes, gradient and diagonal
        NMI_REFINE_UNROLL
        for (int a = 0; a < 6; ++a) {
            if (num[a] == 1) continue;
            if (c[a] < 1 || c[a] > num[a] - 2) {
                flags |= NMI_REFINE_BORDER(a);
                continue;
            }
            const float fp = f[1 + 2 * a], fm = f[2 + 2 * a];
            if (!refine_usable(fp) || !refine_usable(fm)) {
                flags |= NMI_REFINE_HOLE(a);
                continue;
            }
            act[a] = true;
            g[a] = 0.5f * (fp - fm);
            H[a][a] = (fp - f0) + (fm - f0);
        }
        // cross terms
        {
            int p = 0;
            NMI_REFINE_UNROLL
            for (int a = 0; a < 6; ++a) {
                NMI_REFINE_UNROLL
                for (int b = a + 1; b < 6; ++b, ++p) {
                    if (!act[a] || !act[b]) continue;
                    const float fpp = f[13 + 4 * p], fpm = f[14 + 4 * p], fmp = f[15 + 4 * p], fmm = f[16 + 4 * p];
                    if (refine_usable(fpp) && refine_usable(fpm) && refine_usable(fmp) && refine_usable(fmm))
                        H[a][b] = 0.25f * ((fpp - fpm) - (fmp - fmm));
                    else
                        flags |= NMI_REFINE_CROSS_HOLE;
                    H[b][a] = H[a][b];
                }
            }
        }
        // coupled step: A = -H = L D L^T on the active axes, pivots in axis order, every pivot > 0; A x = g
        bool coupled = false, any = false;
        NMI_REFINE_UNROLL
        for (int a = 0; a < 6; ++a) any = any || act[a];
        if (any) {
            float L[6][6], d[6], z[6];
            coupled = true;
            NMI_REFINE_UNROLL
            for (int j = 0; j < 6; ++j) {
                d[j] = 1.0f;
                z[j] = 0.0f;
                NMI_REFINE_UNROLL
                for (int i = 0; i < 6; ++i) L[i][j] = 0.0f;
            }
            NMI_REFINE_UNROLL
            for (int j = 0; j < 6; ++j) {
                if (!act[j] || !coupled) continue;
                float v = -H[j][j];
                NMI_REFINE_UNROLL
                for (int k = 0; k < j; ++k)
                    if (act[k]) v = v - (L[j][k] * d[k]) * L[j][k];
                d[j] = v;
                if (!(v > 0.0f)) {
                    coupled = false;
                    continue;
                }
                NMI_REFINE_UNROLL
                for (int i = j + 1; i < 6; ++i) {
                    if (!act[i]) continue;
                    float w = -H[i][j];
                    NMI_REFINE_UNROLL
                    for (int k = 0; k < j; ++k)
                        if (act[k]) w = w - (L[i][k] * d[k]) * L[j][k];
                    L[i][j] = w / v;
                }
            }
            if (coupled) {
                NMI_REFINE_UNROLL
                for (int i = 0; i < 6; ++i) {  // L z = g, then D y = z
                    if (!act[i]) continue;
                    float v = g[i];
                    NMI_REFINE_UNROLL
                    for (int k = 0; k < i; ++k)
                        if (act[k]) v = v - L[i][k] * z[k];
                    z[i] = v;
                }
                NMI_REFINE_UNROLL
                for (int i = 5; i >= 0; --i) {  // L^T x = y
                    if (!act[i]) continue;
                    float v = z[i] / d[i];
                    NMI_REFINE_UNROLL
                    for (int k = i + 1; k < 6; ++k)
                        if (act[k]) v = v - L[k][i] * x[k];
                    x[i] = v;
                }
                NMI_REFINE_UNROLL
                for (int a = 0; a < 6; ++a)
                    if (act[a] && !(x[a] >= -1.0f && x[a] <= 1.0f)) coupled = false;
            }
        }
        if (coupled) {
            flags |= NMI_REFINE_COUPLED;
        } else {  // separable step
            NMI_REFINE_UNROLL
            for (int a = 0; a < 6; ++a) {
                x[a] = 0.0f;
                if (!act[a]) continue;
                if (H[a][a] < 0.0f) {
                    const float v = (-g[a]) / H[a][a];  // never NaN: g is finite (one difference of finite samples), H < 0 or -inf
                    x[a] = v < -1.0f ? -1.0f : v > 1.0f ? 1.0f : v;
                } else {
                    flags |= NMI_REFINE_FLAT(a);
                }
            }
        }
        // score
        float lin = 0.0f, quad = 0.0f;
        NMI_REFINE_UNROLL
        for (int a = 0; a < 6; ++a) {
            if (!act[a]) continue;
            lin = lin + g[a] * x[a];
            float row = 0.0f;
            NMI_REFINE_UNROLL
            for (int b = 0; b < 6; ++b)
                if (act[b]) row = row + H[a][b] * x[b];
            quad = quad + x[a] * row;
        }
        score = (f0 + lin) + 0.5f * quad;
    }
    r->key = key;
    r->score = score;
    r->flags = flags;
    r->reserved = 0;
    int t = 0;
    NMI_REFINE_UNROLL
    for (int a = 0; a < 6; ++a) {
        r->offset[a] = x[a];
        r->gradient[a] = g[a];
        NMI_REFINE_UNROLL
        for (int b = a; b < 6; ++b, ++t) r->hessian[t] = H[a][b];
    }
}

// The six coordinates of a cell (axis 0 fastest) and the axes' strides; cells = the product of num.
NMI_REFINE_HD void refine_coordinates(uint32_t cell, const int32_t num[6], int32_t c[6], uint32_t stride[6])
{
    uint32_t rem = cell, s = 1;
    NMI_REFINE_UNROLL
    for (int a = 0; a < 6; ++a) {
        c[a] = (int32_t)(rem % (uint32_t)num[a]);
        rem /= (uint32_t)num[a];
        stride[a] = s;
        s *= (uint32_t)num[a];
    }
}

// The shape check every form shares: the number of cells, or 0 for a count < 1, or -1 when the indices do not fit a key's 32 bits.
NMI_REFINE_HD int64_t refine_cells(const int32_t num[6])
{
    int64_t n = 1;
    bool too_many = false;
    for (int a = 0; a < 6; ++a) {
        if (num[a] < 1) return 0;
        n *= num[a];
        if (n >= 0xFFFFFFFFll) too_many = true, n = 0xFFFFFFFFll;
    }
    return too_many ? -1 : n;
}

}  // namespace nmi
