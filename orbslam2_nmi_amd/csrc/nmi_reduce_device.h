// nmi_reduce_device.h -- device code of the box rule of nmi_reduce_frame (include/nmi_hip.h), shared by the reduction kernel
// (nmi_reduce.hip) and the mosaic kernel (nmi_bayer.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nmi {
namespace {

// The rounded mean of F * F grey values from their sum (include/nmi_hip.h): each is within 0.5 of the exact mean, and F = 4
// rounds halves to even.  F = 1: the value itself.
template <int F>
__device__ __forceinline__ uint32_t reduce_round(uint32_t s)
{
    if constexpr (F == 1) {
        return s;
    } else if constexpr (F == 2) {
        return (s + 2u) >> 2;
    } else if constexpr (F == 3) {
        return (s + 4u) / 9u;
    } else {
        const uint32_t q = s >> 4, r = s & 15u;
        return q + ((r > 8u || (r == 8u && (q & 1u))) ? 1u : 0u);
    }
}

}  // namespace
}  // namespace nmi
