// nmi_mask_bits.hip -- bit-packed masks (nmi_mask_bits.h): the unpack that turns a covered stream ticket's render-mask bits
// (1/8 of a render stack on the wire) back into the byte masks the covered search reads, and the pack behind nmi_pack_mask_bits
// for a producer that renders coverage on a GPU and copies only the bits to host memory.
//
// Both are pure streaming kernels, bound by the byte side's traffic.  The unpack writes 8x what it reads: with npix % 16 == 0
// the bits of consecutive images are contiguous (no padding byte), so lane g of the whole launch reads bit bytes 2g and 2g + 1
// and writes pixels 16g .. 16g + 15 with ONE 16-byte store -- a wavefront covers 1 KiB of whole 128-byte lines, where byte or
// dword stores would cost several times the issue per byte.  Other sizes (KITTI's 1241 x 376: npix % 8 == 0 but % 16 != 0,
// odd sizes) take the byte path: one lane per output byte.
#include "nmi_mask_bits.h"

namespace nmi {

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 8192;  // grid-stride beyond this

// bits 0..3 of b -> bytes 0..3 of the word, each 0 or 1 (b * (1 + 2^7 + 2^14 + 2^21): bit k lands at 8k, no carries)
__device__ __forceinline__ uint32_t spread4(uint32_t b) { return ((b & 0xFu) * 0x00204081u) & 0x01010101u; }

__global__ __launch_bounds__(kThreads) void nmi_unpack_bits16_kernel(const uint8_t *__restrict__ bits, size_t groups,
                                                                     uint4 *__restrict__ out)
{
    for (size_t g = (size_t)blockIdx.x * kThreads + threadIdx.x; g < groups; g += (size_t)gridDim.x * kThreads) {
        const uint32_t lo = bits[2 * g], hi = bits[2 * g + 1];
        out[g] = make_uint4(spread4(lo), spread4(lo >> 4), spread4(hi), spread4(hi >> 4));
    }
}

__global__ __launch_bounds__(kThreads) void nmi_unpack_bits1_kernel(const uint8_t *__restrict__ bits, int npix, size_t bytes_per_image,
                                                                    size_t total, uint8_t *__restrict__ out)
{
    for (size_t q = (size_t)blockIdx.x * kThreads + threadIdx.x; q < total; q += (size_t)gridDim.x * kThreads) {
        const size_t i = q / (size_t)npix;
        const uint32_t p = (uint32_t)(q - i * (size_t)npix);
        out[q] = (uint8_t)((bits[i * bytes_per_image + (p >> 3)] >> (p & 7u)) & 1u);
    }
}

// One bit byte per lane.  ALIGNED: npix % 8 == 0 and masks 8-byte aligned, so the lane's 8 mask bytes are one 8-byte load.
template <bool ALIGNED>
__global__ __launch_bounds__(kThreads) void nmi_pack_bits_kernel(const uint8_t *__restrict__ masks, int npix, size_t bytes_per_image,
                                                                 size_t total, uint8_t *__restrict__ bits)
{
    for (size_t q = (size_t)blockIdx.x * kThreads + threadIdx.x; q < total; q += (size_t)gridDim.x * kThreads) {
        const size_t i = q / bytes_per_image;
        const uint32_t j = (uint32_t)(q - i * bytes_per_image);
        const uint8_t *m = masks + i * (size_t)npix + 8u * j;
        uint32_t b = 0;
        if (ALIGNED) {
            const uint2 v = *reinterpret_cast<const uint2 *>(m);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                b |= (uint32_t)(((v.x >> (8 * k)) & 0xFFu) != 0u) << k;
                b |= (uint32_t)(((v.y >> (8 * k)) & 0xFFu) != 0u) << (k + 4);
            }
        } else {
            const uint32_t left = (uint32_t)npix - 8u * j;
            const uint32_t cnt = left < 8u ? left : 8u;
            for (uint32_t k = 0; k < cnt; ++k) b |= (uint32_t)(m[k] != 0) << k;
        }
        bits[q] = (uint8_t)b;
    }
}

unsigned blocks_for(size_t items)
{
    const size_t b = (items + kThreads - 1) / kThreads;
    return (unsigned)(b < (size_t)kMaxBlocks ? b : (size_t)kMaxBlocks);
}

}  // namespace

hipError_t launch_unpack_mask_bits(const uint8_t *bits, int n, int npix, uint8_t *out, hipStream_t stream)
{
    if (n <= 0 || npix <= 0) return hipSuccess;
    if (npix % 16 == 0 && (uintptr_t)out % 16 == 0) {
        const size_t groups = (size_t)n * (size_t)(npix / 16);
        hipLaunchKernelGGL(nmi_unpack_bits16_kernel, dim3(blocks_for(groups)), dim3(kThreads), 0, stream, bits, groups,
                           reinterpret_cast<uint4 *>(out));
    } else {
        const size_t total = (size_t)n * (size_t)npix;
        hipLaunchKernelGGL(nmi_unpack_bits1_kernel, dim3(blocks_for(total)), dim3(kThreads), 0, stream, bits, npix, mask_bit_bytes(npix),
                           total, out);
    }
    return hipGetLastError();
}

hipError_t launch_pack_mask_bits(const uint8_t *masks, int n, int npix, uint8_t *bits, hipStream_t stream)
{
    if (n <= 0 || npix <= 0) return hipSuccess;
    const size_t bpi = mask_bit_bytes(npix), total = (size_t)n * bpi;
    if (npix % 8 == 0 && (uintptr_t)masks % 8 == 0)
        hipLaunchKernelGGL(nmi_pack_bits_kernel<true>, dim3(blocks_for(total)), dim3(kThreads), 0, stream, masks, npix, bpi, total, bits);
    else
        hipLaunchKernelGGL(nmi_pack_bits_kernel<false>, dim3(blocks_for(total)), dim3(kThreads), 0, stream, masks, npix, bpi, total, bits);
    return hipGetLastError();
}

}  // namespace nmi
