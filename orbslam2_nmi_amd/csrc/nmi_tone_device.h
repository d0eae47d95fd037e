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

}  // namespace
}  // namespace nmi
