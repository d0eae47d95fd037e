// nmi_masked_level.hip -- the count and table nodes of a masked level (nmi_level_set_masks, nmi_capi_pipeline.cpp).
//
// A level owns its counts, its previous counts and its per-warp term tables.  Within a strategy level the warps' homographies
// are the same on every replay (the warps rotate the camera frame about identity by the level's fixed steps), so len_w
// repeats from replay to replay and the tables -- fp64 logarithms over Wn x (npix + 1) entries, most of the standalone masked
// search's fixed cost -- need rebuilding only for the warps whose count changed.  The count node marks those warps; the
// table node returns at once for the others.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nmi_mask_device.h"  // kLdsTable, nonzero_byte_bits

namespace nmi {

// One workgroup per warp: nmi_mask_count_kernel's count, then changed[w] = (count != prev[w]), prev[w] = count.
__global__ __launch_bounds__(1024) void nmi_level_mask_count_kernel(const uint8_t *__restrict__ masks, int npix, int32_t *__restrict__ counts,
                                                                   int32_t *__restrict__ prev, int32_t *__restrict__ changed)
{
    __shared__ uint32_t part[16];
    const int w = blockIdx.x, tid = threadIdx.x;
    const uint8_t *m = masks + (size_t)w * npix;
    const int head = min((int)((16u - ((uintptr_t)m & 15u)) & 15u), npix);  // bytes before the first aligned 16-byte unit
    const int units = (npix - head) >> 4;
    uint32_t n = 0;
    for (int i = tid; i < head; i += 1024) n += m[i] != 0;
    const uint4 *u = reinterpret_cast<const uint4 *>(m + head);
    for (int i = tid; i < units; i += 1024) {
        const uint4 v = u[i];
        n += __popc(nonzero_byte_bits(v.x)) + __popc(nonzero_byte_bits(v.y)) + __popc(nonzero_byte_bits(v.z)) + __popc(nonzero_byte_bits(v.w));
    }
    for (int i = head + units * 16 + tid; i < npix; i += 1024) n += m[i] != 0;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) n += (uint32_t)__shfl_xor((int)n, off, 64);
    if ((tid & 63) == 0) part[tid >> 6] = n;
    __syncthreads();
    if (tid == 0) {
        uint32_t t = 0;
        for (int k = 0; k < 16; ++k) t += part[k];
        counts[w] = (int32_t)t;
        changed[w] = prev[w] != (int32_t)t;
        prev[w] = (int32_t)t;
    }
}

// nmi_mask_table_kernel (nmi_masked_kernel.hip) for the warps whose count changed; the same expression, the same entries written.
// Grid-stride over the entries with a bounded grid: a warp whose count did not change costs kTableBlocks workgroups that
// return at once (one workgroup per 256 entries, as nmi_mask_table_kernel launches, took 10 us to dispatch and retire
// 27 x 1,592 empty workgroups at 848 x 480).
constexpr int kTableBlocks = 64;
__global__ __launch_bounds__(256) void nmi_level_mask_table_kernel(const int32_t *__restrict__ counts, const int32_t *__restrict__ changed, int npix,
                                                                   float *__restrict__ tables)
{
    const int w = blockIdx.y;
    if (!changed[w]) return;
    const int len = counts[w];
    float *__restrict__ tw = tables + (size_t)w * ((size_t)npix + 1);
    for (int c = blockIdx.x * blockDim.x + threadIdx.x; c <= npix; c += gridDim.x * blockDim.x) {
        float v = 0.0f;
        if (c > len) {
            if (c >= kLdsTable) break;  // never read: joint and marginal counts are <= len; only the LDS copy reads up to kLdsTable - 1
        } else if (c > 0) {
            const float p = (float)c / (float)len;
            const float l = (float)log2((double)p);
            v = p * l;
        }
        tw[c] = v;
    }
}

hipError_t launch_level_mask_counts(const uint8_t *masks, int Wn, int npix, int32_t *counts, int32_t *prev, int32_t *changed, hipStream_t stream)
{
    hipLaunchKernelGGL(nmi_level_mask_count_kernel, dim3(Wn), dim3(1024), 0, stream, masks, npix, counts, prev, changed);
    return hipGetLastError();
}

hipError_t launch_level_mask_tables(const int32_t *counts, const int32_t *changed, int Wn, int npix, float *tables, hipStream_t stream)
{
    const int threads = 256, blocks = (npix + 1 + threads - 1) / threads;
    hipLaunchKernelGGL(nmi_level_mask_table_kernel, dim3(blocks < kTableBlocks ? blocks : kTableBlocks, Wn), dim3(threads), 0, stream, counts, changed,
                       npix, tables);
    return hipGetLastError();
}

}  // namespace nmi
