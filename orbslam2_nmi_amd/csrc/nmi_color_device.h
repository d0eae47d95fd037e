// nmi_color_device.h -- device code of the colour-to-grey rule (nmi_gray_frame, include/nmi_hip.h), shared by the conversion
// kernel (nmi_color.hip) and by the colour instantiation of the undistortion kernel (nmi_undistort.hip), whose bilinear taps
// convert each source pixel before the fp32 arithmetic of the grey frame.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace nmi {
namespace {

// OpenCV's 8-bit fixed-point COLOR_{RGB,BGR,RGBA,BGRA}2GRAY: the weights 0.299, 0.587, 0.114 in units of 2^-14, rounded.  They
// sum to 2^14, so R = G = B = g gives g exactly.
__device__ __forceinline__ uint32_t color_gray(uint32_t r, uint32_t g, uint32_t b) { return (4899u * r + 9617u * g + 1868u * b + 8192u) >> 14; }

// The grey value of the pixel at p: C bytes per pixel (1: grey, copied; 3 or 4: colour, a fourth byte ignored), R at byte RI
// and B at byte 2 - RI.  C = 2: packed YUV 4:2:2, the luma byte RI (0: YUYV, 1: UYVY) copied, the chroma byte never read.
template <int C, int RI>
__device__ __forceinline__ uint32_t color_pixel(const uint8_t *p)
{
    if constexpr (C == 1)
        return p[0];
    else if constexpr (C == 2)
        return p[RI];
    else
        return color_gray(p[RI], p[1], p[2 - RI]);
}

// Tap fetch of warp_sample_taps (nmi_warp_device.h) on a colour or pitched frame: the grey value of pixel (x, y) of the H rows
// of pitch bytes at src, 0 outside (BORDER_CONSTANT, as warp_tap).
template <int C, int RI>
struct ColorTaps {
    const uint8_t *__restrict__ src;
    size_t pitch;
    __device__ __forceinline__ float operator()(int w, int h, int x, int y) const
    {
        return (x >= 0 && x < w && y >= 0 && y < h) ? (float)color_pixel<C, RI>(src + (size_t)y * pitch + (size_t)x * C) : 0.0f;
    }
};

}  // namespace
}  // namespace nmi
