// nmi_tone_device.h -- device code the deep-frame kernels share (nmi_tone.hip, nmi_clahe.hip): the table kernels' exact quotient,
// the histogram kernels' flush and quarter hand-shake, the masked conversions' mask store, and the arguments of the valid range.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nmi {

// The kernel arguments of the valid range (nmi_tone.h's ValidRange): the ranged histogram kernels take the range, the masked
// conversions the range and the mask pair, the plain instantiations nothing.  A kernel template takes them as a pack of scalar
// arguments -- these members, in this order, or none -- so that each instantiation has the plain argument list of a kernel
// written for it alone, and names them through `const RangeArgs<Ranged> range{lo_hi...}`.
template <bool Ranged>
struct RangeArgs {};
template <>
struct RangeArgs<true> {
    uint32_t lo, hi;
};
template <bool Masked>
struct MaskArgs {};
template <>
struct MaskArgs<true> {
    uint32_t lo, hi;
    const uint8_t *frame_mask;
    uint8_t *mask;
};

namespace {

// floor(num / den) for num < 2^42, 0 < den < 2^32, inv_den = 1.0 / den: the fp64 product is within one of it.
__device__ __forceinline__ uint32_t floor_div(uint64_t num, uint32_t den, double inv_den)
{
    uint64_t q = (uint64_t)((double)num * inv_den);
    if (q * den > num) --q;
    if ((q + 1) * den <= num) ++q;
    return (uint32_t)q;
}

// The histogram kernels' flush of LDS bins 4 i .. 4 i + 3 after a pass: the nonzero ones are added to out's and cleared for the
// next pass.
__device__ __forceinline__ void flush_bins_quad(uint4 *bins4, uint32_t *out, int i)
{
    const uint4 c = bins4[i];
    if (c.x | c.y | c.z | c.w) {
        bins4[i] = make_uint4(0u, 0u, 0u, 0u);
        if (c.x) atomicAdd(&out[4 * i], c.x);
        if (c.y) atomicAdd(&out[4 * i + 1], c.y);
        if (c.z) atomicAdd(&out[4 * i + 2], c.z);
        if (c.w) atomicAdd(&out[4 * i + 3], c.w);
    }
}

// The quarters of the range (v >> 14) any lane of the workgroup has seen a pixel in, bit q each, through the shared word
// *quarters; all lanes call it, and a barrier stands between its return and the next call.
__device__ __forceinline__ uint32_t quarters_present(uint32_t *quarters, uint32_t seen, int tid)
{
    if (tid == 0) *quarters = 0u;
    __syncthreads();
    if (seen) atomicOr(quarters, seen);
    __syncthreads();
    return *quarters;
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
