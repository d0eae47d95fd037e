// ASan/UBSan exercise of nmi_find_peaks (include/nmi_host.h, host/nmi_peaks_host.cpp; no GPU): boxes clipped at the grid's
// corners, a box that covers the whole table, axes of one cell under a radius, huge radii, refused arguments.  Answers are
// literal or follow from the rule by hand.  Built and run by tests/test_peaks_model.py with -fsanitize=address,undefined.
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
            printf("find_peaks.cpp:%d: %s\n", __LINE__, #cond);   \
            return 1;                                             \
        }                                                         \
    } while (0)

int main()
{
    uint64_t keys[64];
    // 1. corners: a 3^6 table whose 64 corners hold 2.0 over a floor of 1.0.  Radius 1: a corner's clipped box is 2^6 cells and
    //    holds no other corner, so the first 64 peaks are the corners in index order.
    {
        const int32_t num[6] = {3, 3, 3, 3, 3, 3}, r1[6] = {1, 1, 1, 1, 1, 1};
        std::vector<float> t(729, 1.0f);
        std::vector<uint32_t> corners;
        for (uint32_t i = 0; i < 729; ++i) {
            bool corner = true;
            for (uint32_t a = 0, rem = i; a < 6; ++a, rem /= 3) corner = corner && rem % 3 != 1;
            if (corner) t[i] = 2.0f, corners.push_back(i);
        }
        CHECK(corners.size() == 64);
        CHECK(nmi_find_peaks(t.data(), num, 64, r1, keys) == 64);
        for (int k = 0; k < 64; ++k) CHECK(keys[k] == key_of(2.0f, corners[(size_t)k]));
        // 2. the box of the first peak covers the whole table
        const int32_t r2[6] = {2, 2, 2, 2, 2, 2};
        CHECK(nmi_find_peaks(t.data(), num, 64, r2, keys) == 1);
        CHECK(keys[0] == key_of(2.0f, 0));
        for (int k = 1; k < 64; ++k) CHECK(keys[k] == 0);
        const int32_t huge[6] = {INT32_MAX, INT32_MAX, INT32_MAX, INT32_MAX, INT32_MAX, INT32_MAX};
        CHECK(nmi_find_peaks(t.data(), num, 7, huge, keys) == 1 && keys[0] == key_of(2.0f, 0) && keys[1] == 0 && keys[6] == 0);
    }
    // 3. axes of one cell under a radius: [1,4,1,1,2,1], radius 1 everywhere.  Ascending scores: the winner is the last cell
    //    (sy 3, wy 1); its box is sy 2..3 x wy 0..1; next comes sy 1, wy 1 (index 5), whose box takes sy 0..2: nothing is left.
    {
        const int32_t num[6] = {1, 4, 1, 1, 2, 1}, r1[6] = {1, 1, 1, 1, 1, 1};
        const float t[8] = {0.1f, 0.2f, 0.3f, 0.4f, 0.5f, 0.6f, 0.7f, 0.8f};
        CHECK(nmi_find_peaks(t, num, 8, r1, keys) == 2);
        CHECK(keys[0] == key_of(0.8f, 7) && keys[1] == key_of(0.6f, 5) && keys[2] == 0 && keys[7] == 0);
        const int32_t r0[6] = {0, 0, 0, 0, 0, 0};
        CHECK(nmi_find_peaks(t, num, 8, r0, keys) == 8);
        for (int k = 0; k < 8; ++k) CHECK(keys[k] == key_of(t[7 - k], (uint32_t)(7 - k)));
    }
    // 4. one cell; nothing qualifies; -0.0 counts as 0.0
    {
        const int32_t one[6] = {1, 1, 1, 1, 1, 1}, r1[6] = {1, 1, 1, 1, 1, 1};
        const float a = 0.25f, b = -0.0f, c = -1.0f, d = NAN;
        CHECK(nmi_find_peaks(&a, one, 2, r1, keys) == 1 && keys[0] == key_of(0.25f, 0) && keys[1] == 0);
        CHECK(nmi_find_peaks(&b, one, 1, r1, keys) == 1 && keys[0] == 0xFFFFFFFFull);
        CHECK(nmi_find_peaks(&c, one, 1, r1, keys) == 0 && keys[0] == 0);
        CHECK(nmi_find_peaks(&d, one, 1, r1, keys) == 0 && keys[0] == 0);
    }
    // 5. refused arguments leave the keys alone
    {
        const int32_t num[6] = {2, 1, 1, 1, 1, 1}, r0[6] = {0, 0, 0, 0, 0, 0}, bad_num[6] = {2, 0, 1, 1, 1, 1}, bad_r[6] = {0, 0, -1, 0, 0, 0};
        const float t[2] = {1.0f, 2.0f};
        keys[0] = 77;
        CHECK(nmi_find_peaks(nullptr, num, 1, r0, keys) == -1 && nmi_find_peaks(t, nullptr, 1, r0, keys) == -1);
        CHECK(nmi_find_peaks(t, num, 1, nullptr, keys) == -1 && nmi_find_peaks(t, num, 1, r0, nullptr) == -1);
        CHECK(nmi_find_peaks(t, num, 0, r0, keys) == -1 && nmi_find_peaks(t, num, 65, r0, keys) == -1);
        CHECK(nmi_find_peaks(t, bad_num, 1, r0, keys) == -1 && nmi_find_peaks(t, num, 1, bad_r, keys) == -1);
        CHECK(keys[0] == 77);
    }
    printf("find peaks ok\n");
    return 0;
}
