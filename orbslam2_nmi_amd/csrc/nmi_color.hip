// nmi_color.hip -- colour and pitched camera frames to the dense grey frame the warps read (nmi_gray_frame, include/nmi_hip.h):
// OpenCV's 8-bit fixed-point COLOR_{RGB,BGR,RGBA,BGRA}2GRAY, gray = (4899 R + 9617 G + 1868 B + 8192) >> 14
// (nmi_color_device.h), a copy of the rows of a pitched grey frame, or the luma bytes of packed YUV 4:2:2 (YUYV, UYVY); Bayer
// mosaics go to nmi_bayer.hip.  The kernel moves a frame's bytes once: at 848x480 RGB
// about 1.2 MB in and 0.4 MB out, so its time is mostly launch cost.  The same rule on each bilinear tap makes the colour
// instantiation of the undistortion kernel (nmi_undistort.hip).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nmi_hip.h"
#include "nmi_color.h"
#include "nmi_color_device.h"

namespace nmi {

namespace {

constexpr int kGrayQuads = 64;  // lanes per block row: 4 x 64 = 256 pixels; 4 block rows (the undistortion kernel's shape)

}  // namespace

// A lane makes 4 adjacent grey pixels of one row.  vec_in: every source row starts on a 4-byte boundary (base and pitch), so a
// whole quad's C * 4 bytes (one dword for grey, 12 bytes for 3 channels, 16 for 4) come in one load; otherwise, and for the
// last quad of a row whose width is not a multiple of 4, byte loads.  vec_out: width % 4 == 0 and gray 4-byte aligned, one
// dword store; otherwise byte stores.
template <int C, int RI>
__global__ __launch_bounds__(256) void nmi_gray_kernel(const uint8_t *__restrict__ src, size_t pitch, uint8_t *__restrict__ gray, int width,
                                                       int height, int vec_in, int vec_out)
{
    const int q = blockIdx.x * kGrayQuads + (int)threadIdx.x;
    const int y = blockIdx.y * 4 + (int)threadIdx.y;
    const int x0 = q * 4;
    if (x0 >= width || y >= height) return;
    const int n = min(4, width - x0);
    const uint8_t *row = src + (size_t)y * pitch + (size_t)x0 * C;
    uint32_t packed = 0;
    if (vec_in && n == 4) {
        uint32_t w[C];  // pixel k's channel c is byte k * C + c
        __builtin_memcpy(w, __builtin_assume_aligned(row, 4), 4 * C);
        uint8_t b[4 * C];
#pragma unroll
        for (int i = 0; i < 4 * C; ++i) b[i] = (uint8_t)(w[i / 4] >> (8 * (i % 4)));
#pragma unroll
        for (int k = 0; k < 4; ++k) packed |= color_pixel<C, RI>(b + k * C) << (8 * k);
    } else {
        for (int k = 0; k < n; ++k) packed |= color_pixel<C, RI>(row + k * C) << (8 * k);
    }
    const size_t o = (size_t)y * width + x0;
    if (vec_out) {  // (width % 4 == 0: the quad lies wholly inside the row)
        *reinterpret_cast<uint32_t *>(gray + o) = packed;
    } else {
        for (int k = 0; k < n; ++k) gray[o + k] = (uint8_t)(packed >> (8 * k));
    }
}

hipError_t launch_gray(const uint8_t *src, int format, int64_t pitch, uint8_t *gray, int width, int height, hipStream_t stream)
{
    const int quads = (width + 3) / 4;
    const dim3 grid((quads + kGrayQuads - 1) / kGrayQuads, (height + 3) / 4), block(kGrayQuads, 4);
    const int vec_in = ((uintptr_t)src % 4) == 0 && (pitch % 4) == 0;
    const int vec_out = (width % 4) == 0 && ((uintptr_t)gray % 4) == 0;
    if (frame_is_bayer(format)) return launch_bayer(src, format, pitch, 1, gray, width, height, stream);
    const size_t pb = (size_t)pitch;
    switch (format) {
    case NMI_FRAME_YUYV:  // (2 bytes per pixel: a quad's 8 bytes in one load)
        hipLaunchKernelGGL((nmi_gray_kernel<2, 0>), grid, block, 0, stream, src, pb, gray, width, height, vec_in, vec_out);
        break;
    case NMI_FRAME_UYVY:
        hipLaunchKernelGGL((nmi_gray_kernel<2, 1>), grid, block, 0, stream, src, pb, gray, width, height, vec_in, vec_out);
        break;
    case NMI_FRAME_GRAY:
        hipLaunchKernelGGL((nmi_gray_kernel<1, 0>), grid, block, 0, stream, src, pb, gray, width, height, vec_in, vec_out);
        break;
    case NMI_FRAME_BGR:
        hipLaunchKernelGGL((nmi_gray_kernel<3, 2>), grid, block, 0, stream, src, pb, gray, width, height, vec_in, vec_out);
        break;
    case NMI_FRAME_RGB:
        hipLaunchKernelGGL((nmi_gray_kernel<3, 0>), grid, block, 0, stream, src, pb, gray, width, height, vec_in, vec_out);
        break;
    case NMI_FRAME_BGRA:
        hipLaunchKernelGGL((nmi_gray_kernel<4, 2>), grid, block, 0, stream, src, pb, gray, width, height, vec_in, vec_out);
        break;
    case NMI_FRAME_RGBA:
        hipLaunchKernelGGL((nmi_gray_kernel<4, 0>), grid, block, 0, stream, src, pb, gray, width, height, vec_in, vec_out);
        break;
    default:
        return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace nmi
