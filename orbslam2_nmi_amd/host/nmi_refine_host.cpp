// nmi_refine_host.cpp -- nmi_refine_peaks_host and nmi_refined_covariance (include/nmi_host.h): the refined-peaks rule of
// include/nmi_hip.h ("Refined peaks") on a host table, and the covariance a record stands for.  Plain C++, no GPU: it links
// without the device library (tests/native/refine_peaks.cpp).  The arithmetic is nmi_refine_rule.h's, the kernel's own.
#include <stdint.h>
#include <string.h>

#include "nmi_host.h"
#include "nmi_refine_rule.h"

extern "C" int64_t nmi_refine_peaks_host(const float *ratings, const int32_t num[6], const uint64_t *keys, int32_t K, nmi_refined_peak *records)
{
    if (!ratings || !num || !keys || !records || K < 1 || K > nmi::kRefineMaxK) return -1;
    const int64_t cells = nmi::refine_cells(num);
    if (cells < 1) return -1;
    int64_t count = 0;
    for (int32_t k = 0; k < K; ++k) {
        nmi_refined_peak *r = records + k;
        const uint32_t centre = 0xFFFFFFFFu - (uint32_t)keys[k];
        if (keys[k] == 0 || (int64_t)centre >= cells) {  // the empty record: the table is not read
            memset(r, 0, sizeof *r);
            r->flags = NMI_REFINE_EMPTY;
            continue;
        }
        int32_t c[6];
        uint32_t stride[6];
        nmi::refine_coordinates(centre, num, c, stride);
        float samples[nmi::kRefineSamples];
        for (int s = 0; s < nmi::kRefineSamples; ++s) samples[s] = ratings[nmi::refine_sample_cell(s, centre, c, num, stride)];
        memset(r, 0, sizeof *r);
        nmi::refine_rule(samples, c, num, keys[k], r);
        ++count;
    }
    return count;
}

extern "C" int nmi_refined_covariance(const nmi_refined_peak *record, const float step[6], double cov[36], uint32_t *active_mask)
{
    if (!record || !step || !cov || !(record->flags & NMI_REFINE_COUPLED)) return -1;
    // A coupled record's -H is positive definite on its active axes, so an active axis has H_aa < 0, and an inactive one H_aa = 0.
    double A[6][6];
    int axis[6], n = 0, t = 0;
    for (int a = 0; a < 6; ++a)
        for (int b = a; b < 6; ++b, ++t) A[a][b] = A[b][a] = -(double)record->hessian[t];
    for (int a = 0; a < 6; ++a)
        if (A[a][a] > 0.0) axis[n++] = a;
    if (n == 0) return -1;
    // L D L^T of the n x n block, then its inverse column by column (symmetrised on the way out)
    double L[6][6] = {}, d[6] = {}, inv[6][6] = {};
    for (int j = 0; j < n; ++j) {
        double v = A[axis[j]][axis[j]];
        for (int k = 0; k < j; ++k) v -= L[j][k] * L[j][k] * d[k];
        if (!(v > 0.0)) return -1;
        d[j] = v;
        L[j][j] = 1.0;
        for (int i = j + 1; i < n; ++i) {
            double w = A[axis[i]][axis[j]];
            for (int k = 0; k < j; ++k) w -= L[i][k] * L[j][k] * d[k];
            L[i][j] = w / v;
        }
    }
    for (int col = 0; col < n; ++col) {
        double z[6], x[6];
        for (int i = 0; i < n; ++i) {
            double v = i == col ? 1.0 : 0.0;
            for (int k = 0; k < i; ++k) v -= L[i][k] * z[k];
            z[i] = v;
        }
        for (int i = n - 1; i >= 0; --i) {
            double v = z[i] / d[i];
            for (int k = i + 1; k < n; ++k) v -= L[k][i] * x[k];
            x[i] = v;
        }
        for (int i = 0; i < n; ++i) inv[i][col] = x[i];
    }
    uint32_t mask = 0;
    for (int i = 0; i < 36; ++i) cov[i] = 0.0;
    for (int i = 0; i < n; ++i) {
        mask |= 1u << axis[i];
        for (int j = 0; j < n; ++j)
            cov[6 * axis[i] + axis[j]] = (double)step[axis[i]] * (double)step[axis[j]] * 0.5 * (inv[i][j] + inv[j][i]);
    }
    if (active_mask) *active_mask = mask;
    return 0;
}
