// nmi_undistort.h -- internal interface of the lens undistortion (nmi_undistort.hip), used by nmi_capi_undistort.cpp
// (nmi_undistort_frame) and by the captured levels and streams of nmi_capi_pipeline.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nmi {

// Lens models (UndistortParams::model; the values of NMI_LENS_* in include/nmi_host.h).
constexpr int kLensRadTan = 0;   // radial-tangential, k1 k2 p1 p2 k3 (nmi_undistort_frame)
constexpr int kLensFisheye = 1;  // Kannala-Brandt equidistant, k1 k2 k3 k4 (nmi_undistort_frame_fisheye)

// The map's fp32 constants, made on the host by nmi_internal::undistort_params / fisheye_params (include/nmi_hip.h,
// nmi_undistort_frame, nmi_undistort_frame_fisheye).
struct UndistortParams {
    float fx, fy, cx, cy;  // fl32 of K[0], K[4], K[2], K[5]; fisheye: of K_raw, the raw frame's camera
    float ifx, ify;        // fl32(1.0 / K[0]), fl32(1.0 / K[4]), computed in double (both models: of the output camera K)
    float k1, k2, p1, p2, k3;
    int model;             // kLensRadTan, kLensFisheye
    float cxn, cyn;        // fisheye: fl32 of K[2], K[5], the output camera's principal point
    float k4;              // fisheye: k1 k2 k3 k4 (p1, p2 unused)
};

// frame[y][x] = the raw frame's bilinear value at the distorted position of (x, y); frame_mask (may be null) = 1 where that
// value comes from taps inside the raw frame (and nonzero in raw_mask, when given), else 0.  raw != frame.
hipError_t launch_undistort(const UndistortParams &p, const uint8_t *raw, const uint8_t *raw_mask, uint8_t *frame, uint8_t *frame_mask,
                            int width, int height, hipStream_t stream);

}  // namespace nmi

namespace nmi_internal {

// K = [fx 0 cx; 0 fy cy; 0 0 1] with finite fx, fy > 0, finite cx, cy; five finite coefficients -> NMI_OK and *out (and
// *identity: all five are zero); else NMI_ERR_INVALID_ARGUMENT.  Touches no device.
int undistort_params(const double K[9], const float dist[5], nmi::UndistortParams *out, bool *identity);
// The fisheye form: K and K_raw (nullptr: K) as above, four finite coefficients k1 k2 k3 k4 -> NMI_OK and *out; else
// NMI_ERR_INVALID_ARGUMENT.  No identity case.  Touches no device.
int fisheye_params(const double K[9], const double K_raw[9], const float dist[4], nmi::UndistortParams *out);

}  // namespace nmi_internal
