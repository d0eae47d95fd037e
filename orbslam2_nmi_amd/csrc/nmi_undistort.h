// nmi_undistort.h -- internal interface of the lens undistortion (nmi_undistort.hip), used by nmi_capi_undistort.cpp
// (nmi_undistort_frame) and by the captured levels and streams of nmi_capi_pipeline.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nmi {

// The map's fp32 constants, made on the host by nmi_internal::undistort_params (include/nmi_hip.h, nmi_undistort_frame).
struct UndistortParams {
    float fx, fy, cx, cy;  // fl32 of K[0], K[4], K[2], K[5]
    float ifx, ify;        // fl32(1.0 / K[0]), fl32(1.0 / K[4]), computed in double
    float k1, k2, p1, p2, k3;
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

}  // namespace nmi_internal
