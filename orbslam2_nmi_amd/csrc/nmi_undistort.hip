// nmi_undistort.hip -- lens undistortion of a camera frame (nmi_undistort_frame, include/nmi_hip.h): the radial-tangential
// model of OpenCV / ORB-SLAM2 (Tracking.cc:133-144 reads k1 k2 p1 p2 [k3]), resampled once per frame onto the pinhole camera
// K the renders use (the new camera matrix is K, as in cv::undistort's default).  Per output pixel (u, v), fp32, in this
// order (the file is built with -ffp-contract=off, so tests/helpers/undistort_np.py reproduces it byte for byte):
//   x = (u - cx) * ifx;  y = (v - cy) * ify;  x2 = x x;  y2 = y y;  xy = x y;  r2 = x2 + y2
//   rad = r2 (k1 + r2 (k2 + r2 k3))
//   dx = ((x rad) + ((2 p1) xy)) + (p2 (r2 + 2 x2));  dy = ((y rad) + (p1 (r2 + 2 y2))) + ((2 p2) xy)
//   xs = u + fx dx;  ys = v + fy dy
// -- the textbook u_d = fx x_d + cx written as a displacement, so that zero coefficients give xs = u, ys = v exactly: the
// frame is copied and every mask byte is 1.  The value at (xs, ys) is warp_sample_global's (nmi_warp_device.h), the mask
// warp_source_valid's: the rules of the warp stack and its masks.  No special case where the polynomial folds over.
// Taps are gathered from global memory (a frame is well under 1 MB and stays in L2); no LDS staging.  The colour instantiation
// (launch_undistort_color) takes its taps from a colour, pitched or packed-YUV frame, converted to grey (nmi_color_device.h)
// one by one; a Bayer mosaic is demosaiced first, in a node of its own (nmi_intake.h).
//
// The fisheye form (nmi_undistort_frame_fisheye): the four-coefficient equidistant model of Kannala-Brandt / cv::fisheye /
// Kalibr "equidistant" / ORB-SLAM3 "KannalaBrandt8".  Two cameras: the output pinhole K (cxn, cyn, ifx, ify) and the raw
// frame's K_raw (fx, fy, cx, cy).  Per output pixel, fp32, in this order (tests/helpers/fisheye_np.py):
//   x = (u - cxn) * ifx;  y = (v - cyn) * ify;  r2 = x x + y y;  r = sqrtf(r2)
//   theta = atan32(r):  big = r > 2.414213562373095f;  mid = !big && r > 0.4142135623730950f
//       a = big ? -1 / r : mid ? (r - 1) / (r + 1) : r;  base = big ? fl32(pi/2) : mid ? fl32(pi/4) : 0;  z = a a
//       q = ((8.05374449538e-2f z - 1.38776856032e-1f) z + 1.99777106478e-1f) z - 3.33329491539e-1f
//       theta = base + ((q z) a + a)
//   t2 = theta theta;  td = theta + theta (t2 (k1 + t2 (k2 + t2 (k3 + t2 k4))))
//   s = r > 1e-8f ? td / r : 1;  xs = cx + fx (x s);  ys = cy + fy (y s)
// The arctangent is spelled out (the single-precision Cephes reduction and polynomial) and atanf is not called: its device
// and host forms differ in the last bit, which flips bytes at rounding ties.  sqrtf and the divisions are the correctly
// rounded sequences hipcc emits by default.  No identity case: zero coefficients are an ideal equidistant lens, still a remap.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "nmi_hip.h"
#include "nmi_color.h"
#include "nmi_color_device.h"
#include "nmi_undistort.h"
#include "nmi_warp_device.h"

namespace nmi {

namespace {

constexpr int kUndistortQuads = 64;  // lanes per block row: 4 x 64 = 256 pixels; 4 block rows

__device__ __forceinline__ void undistort_source(const UndistortParams &p, float u, float v, float *xs, float *ys)
{
    const float x = (u - p.cx) * p.ifx, y = (v - p.cy) * p.ify;
    const float x2 = x * x, y2 = y * y, xy = x * y, r2 = x2 + y2;
    const float rad = r2 * (p.k1 + r2 * (p.k2 + r2 * p.k3));
    const float dx = ((x * rad) + ((2.0f * p.p1) * xy)) + (p.p2 * (r2 + 2.0f * x2));
    const float dy = ((y * rad) + (p.p1 * (r2 + 2.0f * y2))) + ((2.0f * p.p2) * xy);
    *xs = u + p.fx * dx;
    *ys = v + p.fy * dy;
}

// atan(r) for r >= 0 in + - * / and selects, so that numpy float32 reproduces it bit for bit.
__device__ __forceinline__ float atan32(float r)
{
    const bool big = r > 2.414213562373095f;            // tan(3 pi / 8)
    const bool mid = !big && r > 0.4142135623730950f;   // tan(pi / 8)
    const float a = big ? -1.0f / r : mid ? (r - 1.0f) / (r + 1.0f) : r;
    const float base = big ? 1.5707963267948966f : mid ? 0.7853981633974483f : 0.0f;
    const float z = a * a;
    const float q = ((8.05374449538e-2f * z - 1.38776856032e-1f) * z + 1.99777106478e-1f) * z - 3.33329491539e-1f;
    return base + ((q * z) * a + a);
}

__device__ __forceinline__ void fisheye_source(const UndistortParams &p, float u, float v, float *xs, float *ys)
{
    const float x = (u - p.cxn) * p.ifx, y = (v - p.cyn) * p.ify;
    const float r2 = x * x + y * y;
    const float r = sqrtf(r2);
    const float theta = atan32(r);
    const float t2 = theta * theta;
    const float td = theta + theta * (t2 * (p.k1 + t2 * (p.k2 + t2 * (p.k3 + t2 * p.k4))));
    const float s = r > 1e-8f ? td / r : 1.0f;
    *xs = p.cx + p.fx * (x * s);
    *ys = p.cy + p.fy * (y * s);
}

}  // namespace

// A lane makes 4 adjacent pixels of one row (and their mask bytes): one dword store each where every row starts on a 4-byte
// boundary (aligned), byte stores otherwise.  raw fetches the raw frame's grey taps (warp_sample_taps): GrayTaps
// (nmi_warp_device.h) for a dense grey frame (launch_undistort), ColorTaps (nmi_color_device.h) for a colour, pitched or
// packed-YUV one (launch_undistort_color: one node instead of launch_gray followed by this kernel, with the same bytes, each
// tap being the grey value launch_gray would have stored).  Model (kLensRadTan, kLensFisheye) chooses the map from (u, v) to the source coordinate.
template <class Taps, int Model>
__global__ __launch_bounds__(256) void nmi_undistort_kernel(UndistortParams p, const Taps raw, const uint8_t *__restrict__ raw_mask,
                                                            uint8_t *__restrict__ frame, uint8_t *__restrict__ frame_mask, int width, int height,
                                                            int aligned)
{
    const int q = blockIdx.x * kUndistortQuads + (int)threadIdx.x;
    const int y = blockIdx.y * 4 + (int)threadIdx.y;
    const int x0 = q * 4;
    if (x0 >= width || y >= height) return;
    const int n = min(4, width - x0);
    uint32_t packed = 0, mpacked = 0;
    const float v = (float)y;
    for (int k = 0; k < n; ++k) {
        float xs, ys;
        if (Model == kLensFisheye)
            fisheye_source(p, (float)(x0 + k), v, &xs, &ys);
        else
            undistort_source(p, (float)(x0 + k), v, &xs, &ys);
        packed |= warp_sample_taps(raw, width, height, xs, ys) << (8 * k);
        if (frame_mask) mpacked |= (uint32_t)warp_source_valid(raw_mask, width, height, xs, ys) << (8 * k);
    }
    const size_t o = (size_t)y * width + x0;
    if (aligned) {  // (width % 4 == 0: the quad lies wholly inside the row)
        *reinterpret_cast<uint32_t *>(frame + o) = packed;
        if (frame_mask) *reinterpret_cast<uint32_t *>(frame_mask + o) = mpacked;
    } else {
        for (int k = 0; k < n; ++k) frame[o + k] = (uint8_t)(packed >> (8 * k));
        if (frame_mask)
            for (int k = 0; k < n; ++k) frame_mask[o + k] = (uint8_t)(mpacked >> (8 * k));
    }
}

static dim3 undistort_grid(int width, int height)
{
    const int quads = (width + 3) / 4;
    return dim3((quads + kUndistortQuads - 1) / kUndistortQuads, (height + 3) / 4);
}

template <class Taps>
static void launch_model(const UndistortParams &p, const Taps raw, const uint8_t *raw_mask, uint8_t *frame, uint8_t *frame_mask, int width,
                         int height, int aligned, hipStream_t stream)
{
    const dim3 grid = undistort_grid(width, height), block(kUndistortQuads, 4);
    if (p.model == kLensFisheye)
        hipLaunchKernelGGL((nmi_undistort_kernel<Taps, kLensFisheye>), grid, block, 0, stream, p, raw, raw_mask, frame, frame_mask, width, height, aligned);
    else
        hipLaunchKernelGGL((nmi_undistort_kernel<Taps, kLensRadTan>), grid, block, 0, stream, p, raw, raw_mask, frame, frame_mask, width, height, aligned);
}

hipError_t launch_undistort(const UndistortParams &p, const uint8_t *raw, const uint8_t *raw_mask, uint8_t *frame, uint8_t *frame_mask,
                            int width, int height, hipStream_t stream)
{
    const int aligned = (width % 4) == 0 && ((uintptr_t)frame % 4) == 0 && ((uintptr_t)frame_mask % 4) == 0;
    launch_model(p, GrayTaps{raw}, raw_mask, frame, frame_mask, width, height, aligned, stream);
    return hipGetLastError();
}

hipError_t launch_undistort_color(const UndistortParams &p, const uint8_t *src, int format, int64_t pitch, const uint8_t *raw_mask,
                                  uint8_t *frame, uint8_t *frame_mask, int width, int height, hipStream_t stream)
{
    const int aligned = (width % 4) == 0 && ((uintptr_t)frame % 4) == 0 && ((uintptr_t)frame_mask % 4) == 0;
    const size_t pb = (size_t)pitch;
    switch (format) {
    case NMI_FRAME_YUYV:
        launch_model(p, ColorTaps<2, 0>{src, pb}, raw_mask, frame, frame_mask, width, height, aligned, stream);
        break;
    case NMI_FRAME_UYVY:
        launch_model(p, ColorTaps<2, 1>{src, pb}, raw_mask, frame, frame_mask, width, height, aligned, stream);
        break;
    case NMI_FRAME_GRAY:
        launch_model(p, ColorTaps<1, 0>{src, pb}, raw_mask, frame, frame_mask, width, height, aligned, stream);
        break;
    case NMI_FRAME_BGR:
        launch_model(p, ColorTaps<3, 2>{src, pb}, raw_mask, frame, frame_mask, width, height, aligned, stream);
        break;
    case NMI_FRAME_RGB:
        launch_model(p, ColorTaps<3, 0>{src, pb}, raw_mask, frame, frame_mask, width, height, aligned, stream);
        break;
    case NMI_FRAME_BGRA:
        launch_model(p, ColorTaps<4, 2>{src, pb}, raw_mask, frame, frame_mask, width, height, aligned, stream);
        break;
    case NMI_FRAME_RGBA:
        launch_model(p, ColorTaps<4, 0>{src, pb}, raw_mask, frame, frame_mask, width, height, aligned, stream);
        break;
    default:
        return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace nmi
