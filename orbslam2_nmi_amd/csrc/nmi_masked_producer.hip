// nmi_masked_producer.hip -- the warp masks that go with a warp stack (nmi_warp_stack_masked): which pixels of each warp
// were interpolated from inside the camera frame.
//
// warpPerspective with BORDER_CONSTANT 0 (nmi_producers.hip) gives a pixel whose source lies (partly) outside the frame an
// invented value: 0, or a blend of frame taps with 0.  Such pixels are not part of the overlap of frame and render and
// should not enter the histogram (NMI is overlap-invariant only if they are left out).  Pixel (x, y) of warp w is VALID when
//   - the source test of the warp passes: -2 < xs < W + 1 and -2 < ys < H + 1, with xs, ys the fp32 source coordinates
//     computed exactly as warp_pixel_global (nmi_warp_device.h) computes them, in the same order;
//   - every bilinear tap with nonzero weight lies inside the frame: x1 = floor(xs) >= 0, x1 + (xs != x1) <= W - 1, and the
//     same for rows (tap x1 + 1 has weight xs - x1, zero exactly when xs is an integer);
//   - given a frame mask, every such tap is nonzero in it.
// Under the identity homography xs = x and ys = y exactly, so every pixel is valid (and the warp equals the frame).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "nmi_masked.h"
#include "nmi_warp_device.h"

namespace nmi {

namespace {

__device__ __forceinline__ uint8_t warp_pixel_valid(const uint8_t *__restrict__ frame_mask, const float *__restrict__ c, int width,
                                                    int height, int x, int y)
{
    const float fx = (float)x, fy = (float)y;
    const float coeff = 1.0f / (c[6] * fx + c[7] * fy + c[8]);
    const float xs = coeff * (c[0] * fx + c[1] * fy + c[2]);
    const float ys = coeff * (c[3] * fx + c[4] * fy + c[5]);
    return warp_source_valid(frame_mask, width, height, xs, ys);
}

}  // namespace

// One lane per output pixel; a block is 64 x 4 pixels of one warp.
__global__ __launch_bounds__(256) void nmi_warp_mask_kernel(const uint8_t *__restrict__ frame_mask, const float *__restrict__ coeffs,
                                                            uint8_t *__restrict__ out, int width, int height)
{
    const int x = blockIdx.x * 64 + (int)threadIdx.x;
    const int y = blockIdx.y * 4 + (int)threadIdx.y;
    const int wi = blockIdx.z;
    if (x >= width || y >= height) return;
    out[((size_t)wi * height + y) * width + x] = warp_pixel_valid(frame_mask, coeffs + wi * 9, width, height, x, y);
}

hipError_t launch_warp_masks(const uint8_t *frame_mask, const float *coeffs, uint8_t *out_masks, int width, int height, int Wn,
                             hipStream_t stream)
{
    hipLaunchKernelGGL(nmi_warp_mask_kernel, dim3((width + 63) / 64, (height + 3) / 4, Wn), dim3(64, 4), 0, stream, frame_mask, coeffs,
                       out_masks, width, height);
    return hipGetLastError();
}

}  // namespace nmi
