// nmi_tone_device.h -- device code the tone table kernels share (nmi_tone.hip, nmi_clahe.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nmi {
namespace {

// floor(num / den) for num < 2^42, 0 < den < 2^32, inv_den = 1.0 / den: the fp64 product is within one of it.
__device__ __forceinline__ uint32_t floor_div(uint64_t num, uint32_t den, double inv_den)
{
    uint64_t q = (uint64_t)((double)num * inv_den);
    if (q * den > num) --q;
    if ((q + 1) * den <= num) ++q;
    return (uint32_t)q;
}

// The masked conversions' second output: the n (1 .. 4) pixels of the validity mask at mask + o.  bad, bit k: a source pixel of
// output pixel k is outside the valid range.  Pixel k is 1 iff it is not bad and, with a frame mask, frame_mask[o + k] != 0.  The
// frame mask's bytes are read before the mask's are written, so the two may be one buffer.  vec: n == 4 and both 4-byte aligned
// at o, one dword each way.
__device__ __forceinline__ void write_valid_quad(uint32_t bad, const uint8_t *frame_mask, uint8_t *mask, size_t o, int n, int vec)
{
    uint32_t good = ~bad & 15u;
    if (vec) {
        if (frame_mask) {
            const uint32_t f = *reinterpret_cast<const uint32_t *>(frame_mask + o);
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (((f >> (8 * k)) & 255u) == 0u) good &= ~(1u << k);
        }
        // bit k -> byte k: 0x00204081 moves bits 0 .. 3 to bits 0, 8, 16, 24 (no two partial products meet)
        *reinterpret_cast<uint32_t *>(mask + o) = (good * 0x00204081u) & 0x01010101u;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)  // (byte k of the mask depends on byte k of the frame mask alone)
            if (k < n) mask[o + k] = (uint8_t)(((good >> k) & 1u) && (!frame_mask || frame_mask[o + k] != 0));
    }
}

}  // namespace
}  // namespace nmi
