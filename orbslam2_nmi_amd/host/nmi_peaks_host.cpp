// nmi_peaks_host.cpp -- nmi_find_peaks (include/nmi_host.h): the ranked-peaks rule of include/nmi_hip.h ("Ranked peaks") on a
// host table, next to nmi_find_max_elements.  Plain C++, no GPU; it shares nothing with the kernel (nmi_peaks.hip) but the rule.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "nmi_host.h"

namespace {

// nmi_key_pack of include/nmi_hip.h (this file links without the device library: tests/native/find_peaks.cpp)
uint64_t key_of(float score, int64_t index)
{
    if (!(score >= 0.0f)) return 0;
    uint32_t bits = 0;
    if (score != 0.0f) memcpy(&bits, &score, sizeof bits);
    return ((uint64_t)bits << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)index);
}

}  // namespace

extern "C" int64_t nmi_find_peaks(const float *ratings, const int32_t num[6], int32_t K, const int32_t radius[6], uint64_t *keys)
{
    if (!ratings || !num || !radius || !keys || K < 1 || K > 64) return -1;
    int64_t n = 1;
    for (int a = 0; a < 6; ++a) {
        if (num[a] < 1 || radius[a] < 0) return -1;
        n *= num[a];
        if (n >= 0xFFFFFFFFll) return -1;  // the index lives in 32 bits of the key
    }
    std::vector<uint8_t> out((size_t)n, 0);  // cells inside the box of an earlier peak
    int64_t count = 0;
    for (; count < K; ++count) {
        uint64_t best = 0;
        for (int64_t i = 0; i < n; ++i) {
            const uint64_t k = out[(size_t)i] ? 0 : key_of(ratings[i], i);
            if (k > best) best = k;
        }
        if (best == 0) break;
        keys[count] = best;
        // the box around the peak, clipped: an odometer over the six axes, axis 0 fastest
        int64_t rem = (int64_t)(0xFFFFFFFFu - (uint32_t)best), stride[6], lo[6], hi[6], at[6], s = 1;
        for (int a = 0; a < 6; ++a) {
            const int64_t c = rem % num[a], r = radius[a] < num[a] ? radius[a] : num[a];
            rem /= num[a];
            lo[a] = c - r < 0 ? 0 : c - r;
            hi[a] = c + r > num[a] - 1 ? num[a] - 1 : c + r;
            at[a] = lo[a];
            stride[a] = s;
            s *= num[a];
        }
        for (bool more = true; more;) {
            int64_t cell = 0;
            for (int a = 0; a < 6; ++a) cell += at[a] * stride[a];
            out[(size_t)cell] = 1;
            more = false;
            for (int a = 0; a < 6 && !more; ++a) {
                if (at[a] < hi[a]) ++at[a], more = true;
                else at[a] = lo[a];
            }
        }
    }
    for (int64_t k = count; k < K; ++k) keys[k] = 0;
    return count;
}
