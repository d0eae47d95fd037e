// nmi_peaks.h -- internal: ranked peaks of a rating table (include/nmi_hip.h, "Ranked peaks"; nmi_peaks.hip).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

namespace nmi {

constexpr int kPeaksMaxK = 64;          // keys per call
constexpr int kPeaksMaxCells = 65536;   // cells of the largest table one workgroup ranks

// One call: the table, its shape (axis order of nmi_host.h; cells = the product of num, at most kPeaksMaxCells), K in
// 1..kPeaksMaxK, the radii (each already clamped to its axis' num - 1) and where the K keys go: a device array, a mapped host
// array, or both.  post (optional, mapped host memory): receives seq once the keys are written, for a host that polls.
struct PeaksArgs {
    const float *ratings = nullptr;
    int32_t num[6] = {1, 1, 1, 1, 1, 1};
    int32_t radius[6] = {0, 0, 0, 0, 0, 0};
    int32_t cells = 0, K = 0;
    unsigned long long *out = nullptr, *out_host = nullptr, *post = nullptr;
    unsigned long long seq = 0;
};

// The shape check nmi_rank_peaks and nmi_level_set_peaks share: fills a.num, a.radius (clamped), a.cells.
// Returns 0, -1 for a count < 1 or a negative radius, -2 for more than kPeaksMaxCells cells.
inline int peaks_shape(const int32_t num[6], const int32_t radius[6], PeaksArgs &a)
{
    long long cells = 1;
    bool too_many = false;
    for (int i = 0; i < 6; ++i) {
        if (num[i] < 1 || radius[i] < 0) return -1;
        cells *= num[i];
        if (cells > kPeaksMaxCells) too_many = true, cells = kPeaksMaxCells + 1;
        a.num[i] = num[i];
        a.radius[i] = radius[i] < num[i] - 1 ? radius[i] : num[i] - 1;
    }
    if (too_many) return -2;
    a.cells = (int32_t)cells;
    return 0;
}

hipError_t launch_peaks(const PeaksArgs &a, hipStream_t stream);

}  // namespace nmi
