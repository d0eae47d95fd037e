// nmi_depth.hip -- nmi_depth_shade_apply: the depth shade (nmi_depth_device.h) on an array of 24-bit depths.  The renderers'
// depth forms apply the same function to the winners of their pixels (nmi_producers.hip, nmi_mesh.hip); this kernel lets a
// caller with a depth buffer of its own use the rule, and a test hold it to its numpy twin over all 2^24 depths in one call.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nmi_depth_device.h"

namespace nmi {

// One depth per lane and step; bits above the 24th are ignored.
__global__ __launch_bounds__(256) void nmi_depth_apply_kernel(DepthShade shade, const uint32_t *__restrict__ depth24, long long n,
                                                              uint16_t *__restrict__ v_out, uint8_t *__restrict__ grey_out)
{
    const long long step = (long long)gridDim.x * blockDim.x;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += step) {
        uint32_t v, grey;
        depth_shade(shade, depth24[i] & 0xFFFFFFu, v, grey);
        if (v_out) v_out[i] = (uint16_t)v;
        if (grey_out) grey_out[i] = (uint8_t)grey;
    }
}

hipError_t launch_depth_shade_apply(const DepthShade &shade, const uint32_t *depth24, long long n, uint16_t *v, uint8_t *grey, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    const long long blocks = (n + 255) / 256;
    hipLaunchKernelGGL(nmi_depth_apply_kernel, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(256), 0, stream, shade, depth24, n, v, grey);
    return hipGetLastError();
}

}  // namespace nmi
