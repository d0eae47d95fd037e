// ASan/UBSan exercise of nmi_refine_peaks_host, nmi_refined_covariance (host/nmi_refine_host.cpp) and
// nmi_calculate_relocalization_offset (host/nmi_driver.cpp), all of include/nmi_host.h; no GPU.  Peaks on every corner of a grid
// (a stencil that must not leave the table on any axis), a peak at the end of a row beside a planted value in the next row, tables
// allocated to their exact size so that a sample outside them is a report, keys that name no cell, refused arguments.  Answers are
// literal or follow from the rule by hand.  Built and run by tests/test_refine_model.py with -fsanitize=address,undefined.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "nmi_host.h"

static uint64_t key_of(float score, uint32_t index)
{
    uint32_t bits;
    memcpy(&bits, &score, sizeof bits);
    return ((uint64_t)bits << 32) | (uint64_t)(0xFFFFFFFFu - index);
}

#define CHECK(cond)                                               \
    do {                                                          \
        if (!(cond)) {                                            \
            printf("refine_peaks.cpp:%d: %s\n", __LINE__, #cond); \
            return 1;                                             \
        }                                                         \
    } while (0)

static bool all_zero(const void *p, size_t n)
{
    for (size_t i = 0; i < n; ++i)
        if (((const unsigned char *)p)[i]) return false;
    return true;
}

int main()
{
    CHECK(sizeof(nmi_refined_peak) == 152);
    // 1. every cell of a 3^6 table as the peak, the 64 corners among them, on a heap table of exactly 729 floats: no sample may
    //    leave it.  A border axis is flagged; the centre cell (all six active) of a constant table is flat on every axis.
    {
        const int32_t num[6] = {3, 3, 3, 3, 3, 3};
        std::vector<float> t(729, 0.5f);
        std::vector<nmi_refined_peak> rec(64);
        for (uint32_t base = 0; base < 729; base += 64) {
            uint64_t keys[64];
            const int K = base + 64 <= 729 ? 64 : (int)(729 - base);
            for (int k = 0; k < K; ++k) keys[k] = key_of(0.5f, base + (uint32_t)k);
            CHECK(nmi_refine_peaks_host(t.data(), num, keys, K, rec.data()) == K);
            for (int k = 0; k < K; ++k) {
                uint32_t want = 0;
                for (uint32_t a = 0, rem = base + (uint32_t)k; a < 6; ++a, rem /= 3) want |= rem % 3 != 1 ? NMI_REFINE_BORDER(a) : NMI_REFINE_FLAT(a);
                CHECK(rec[(size_t)k].key == keys[k] && rec[(size_t)k].flags == want && rec[(size_t)k].score == 0.5f);
                CHECK(all_zero(rec[(size_t)k].offset, sizeof rec[0].offset) && rec[(size_t)k].reserved == 0);
            }
        }
    }
    // 2. a 1-D parabola 0.9 - 0.01 (x - 1.25)^2 on three cells: offset 0.25, score 0.9, H = -0.02; its covariance 1 / 0.02 * step^2
    {
        const int32_t num[6] = {3, 1, 1, 1, 1, 1};
        float t[3];
        for (int x = 0; x < 3; ++x) t[x] = (float)(0.9 - 0.01 * (x - 1.25) * (x - 1.25));
        const uint64_t key = key_of(t[1], 1);
        nmi_refined_peak r;
        CHECK(nmi_refine_peaks_host(t, num, &key, 1, &r) == 1);
        CHECK(r.flags == NMI_REFINE_COUPLED && fabsf(r.offset[0] - 0.25f) < 1e-4f && fabsf(r.score - 0.9f) < 1e-6f);
        CHECK(fabsf(r.hessian[0] + 0.02f) < 1e-6f && all_zero(r.offset + 1, 5 * sizeof(float)) && all_zero(r.hessian + 1, 20 * sizeof(float)));
        const float step[6] = {0.2f, 1, 1, 1, 1, 1};
        double cov[36];
        uint32_t mask = 99;
        CHECK(nmi_refined_covariance(&r, step, cov, &mask) == 0 && mask == 1u);
        CHECK(fabs(cov[0] - (double)step[0] * step[0] / -(double)r.hessian[0]) < 1e-12 && all_zero(cov + 1, 35 * sizeof(double)));
        // a separable record has no covariance, and the outputs stay as they were
        nmi_refined_peak flat = r;
        flat.flags = NMI_REFINE_FLAT(0);
        cov[0] = 7.0, mask = 99;
        CHECK(nmi_refined_covariance(&flat, step, cov, &mask) == -1 && cov[0] == 7.0 && mask == 99);
        CHECK(nmi_refined_covariance(nullptr, step, cov, &mask) == -1 && nmi_refined_covariance(&r, nullptr, cov, &mask) == -1);
        CHECK(nmi_refined_covariance(&r, step, nullptr, &mask) == -1 && nmi_refined_covariance(&r, step, cov, nullptr) == 0);
    }
    // 3. the end of a row: on (4, 3) the peak at sx = 3 of row 0 (index 3) is a border cell of axis 0 and of axis 1; the value
    //    planted at sx = 0 of row 1 (index 4, its linear neighbour) is not looked at
    {
        const int32_t num[6] = {4, 3, 1, 1, 1, 1};
        std::vector<float> t(12, 0.1f);
        t[3] = 0.9f;
        const uint64_t key = key_of(0.9f, 3);
        nmi_refined_peak a, b;
        CHECK(nmi_refine_peaks_host(t.data(), num, &key, 1, &a) == 1);
        t[4] = 1e30f;
        CHECK(nmi_refine_peaks_host(t.data(), num, &key, 1, &b) == 1);
        CHECK(memcmp(&a, &b, sizeof a) == 0 && a.flags == (NMI_REFINE_BORDER(0) | NMI_REFINE_BORDER(1)) && a.score == 0.9f);
    }
    // 4. keys that name no cell, and the key 0: empty records, nothing read (the table pointer is one float)
    {
        const int32_t num[6] = {1, 1, 1, 1, 1, 1};
        const float one = 0.25f;
        const uint64_t keys[4] = {0, key_of(1.0f, 1), key_of(1.0f, 0xFFFFFFFEu), key_of(0.25f, 0)};
        nmi_refined_peak r[4];
        CHECK(nmi_refine_peaks_host(&one, num, keys, 4, r) == 1);
        for (int k = 0; k < 3; ++k) {
            CHECK(r[k].flags == NMI_REFINE_EMPTY);
            r[k].flags = 0;
            CHECK(all_zero(&r[k], sizeof r[k]));
        }
        CHECK(r[3].key == keys[3] && r[3].flags == 0 && r[3].score == 0.25f);
        // an infinite centre
        const float inf = INFINITY;
        const uint64_t kinf = key_of(inf, 0);
        CHECK(nmi_refine_peaks_host(&inf, num, &kinf, 1, r) == 1 && r[0].flags == NMI_REFINE_NONFINITE && r[0].score == inf);
    }
    // 5. refused arguments leave the records alone
    {
        const int32_t num[6] = {2, 1, 1, 1, 1, 1}, bad_num[6] = {2, 0, 1, 1, 1, 1}, big[6] = {65536, 65536, 1, 1, 1, 1};
        const float t[2] = {1.0f, 2.0f};
        const uint64_t key = key_of(2.0f, 1);
        nmi_refined_peak r;
        memset(&r, 0x5A, sizeof r);
        const nmi_refined_peak was = r;
        CHECK(nmi_refine_peaks_host(nullptr, num, &key, 1, &r) == -1 && nmi_refine_peaks_host(t, nullptr, &key, 1, &r) == -1);
        CHECK(nmi_refine_peaks_host(t, num, nullptr, 1, &r) == -1 && nmi_refine_peaks_host(t, num, &key, 1, nullptr) == -1);
        CHECK(nmi_refine_peaks_host(t, num, &key, 0, &r) == -1 && nmi_refine_peaks_host(t, num, &key, 65, &r) == -1);
        CHECK(nmi_refine_peaks_host(t, bad_num, &key, 1, &r) == -1 && nmi_refine_peaks_host(t, big, &key, 1, &r) == -1);
        CHECK(memcmp(&r, &was, sizeof r) == 0);
    }
    // 6. the pose of a real-valued cell: a zero offset is nmi_calculate_relocalization on every bit; half a cell on a translation
    //    axis moves the pose half a step along that axis' direction; NULL arguments are refused
    {
        nmi_search_kernel k;
        nmi_sk_init(&k);
        const int32_t num[6] = {3, 3, 3, 3, 3, 3}, best[6] = {2, 0, 1, 1, 2, 0};
        const float step[6] = {0.2f, 0.3f, 0.5f, 0.02f, 0.03f, 0.05f};
        memcpy(k.num, num, sizeof num), memcpy(k.best, best, sizeof best), memcpy(k.step, step, sizeof step);
        float Twc[16] = {1, 0, 0, 0.5f, 0, 1, 0, -1.0f, 0, 0, 1, 2.0f, 0, 0, 0, 1};
        float whole[16], zero[16], half[16];
        const float none[6] = {0, 0, 0, 0, 0, 0}, off[6] = {0, 0.5f, 0, 0, 0, 0};
        CHECK(nmi_calculate_relocalization(Twc, &k, whole) == 0 && nmi_calculate_relocalization_offset(Twc, &k, none, zero) == 0);
        CHECK(memcmp(whole, zero, sizeof whole) == 0);
        CHECK(nmi_calculate_relocalization_offset(Twc, &k, off, half) == 0);
        // dir_y is the pose's second column, (0, 1, 0) here
        CHECK(fabsf(half[7] - whole[7] - 0.15f) < 1e-6f && fabsf(half[3] - whole[3]) < 1e-6f && fabsf(half[11] - whole[11]) < 1e-6f);
        CHECK(nmi_calculate_relocalization_offset(nullptr, &k, off, half) == -1 && nmi_calculate_relocalization_offset(Twc, nullptr, off, half) == -1);
        CHECK(nmi_calculate_relocalization_offset(Twc, &k, nullptr, half) == -1 && nmi_calculate_relocalization_offset(Twc, &k, off, nullptr) == -1);
    }
    printf("refine peaks ok\n");
    return 0;
}
