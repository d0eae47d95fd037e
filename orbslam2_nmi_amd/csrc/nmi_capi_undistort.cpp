// nmi_capi_undistort.cpp -- nmi_undistort_frame (include/nmi_hip.h) and the host side of the lens model the captured levels and
// streams share (nmi_level_set_distortion, nmi_stream_set_distortion: both through nmi_capi_intake.cpp's intake_set_distortion
// and launch_intake).  Kernel: nmi_undistort.hip.
#include "nmi_ctx.h"
#include "nmi_undistort.h"

using namespace nmi_internal;

int nmi_internal::undistort_params(const double K[9], const float dist[5], nmi::UndistortParams *out, bool *identity)
{
    if (!K || !dist || !out) return NMI_ERR_INVALID_ARGUMENT;
    for (int i = 0; i < 9; ++i)
        if (!std::isfinite(K[i])) return NMI_ERR_INVALID_ARGUMENT;
    // a pinhole camera without skew: [fx 0 cx; 0 fy cy; 0 0 1]
    if (K[1] != 0.0 || K[3] != 0.0 || K[6] != 0.0 || K[7] != 0.0 || K[8] != 1.0 || !(K[0] > 0.0) || !(K[4] > 0.0)) return NMI_ERR_INVALID_ARGUMENT;
    for (int i = 0; i < 5; ++i)
        if (!std::isfinite(dist[i])) return NMI_ERR_INVALID_ARGUMENT;
    nmi::UndistortParams p{};
    p.fx = (float)K[0], p.fy = (float)K[4], p.cx = (float)K[2], p.cy = (float)K[5];
    p.ifx = (float)(1.0 / K[0]), p.ify = (float)(1.0 / K[4]);
    const float f[6] = {p.fx, p.fy, p.cx, p.cy, p.ifx, p.ify};
    for (float v : f)
        if (!std::isfinite(v)) return NMI_ERR_INVALID_ARGUMENT;
    if (!(p.fx > 0.0f) || !(p.fy > 0.0f) || !(p.ifx > 0.0f) || !(p.ify > 0.0f)) return NMI_ERR_INVALID_ARGUMENT;  // (fl32 under- / overflow)
    p.k1 = dist[0], p.k2 = dist[1], p.p1 = dist[2], p.p2 = dist[3], p.k3 = dist[4];
    *out = p;
    if (identity) *identity = dist[0] == 0.0f && dist[1] == 0.0f && dist[2] == 0.0f && dist[3] == 0.0f && dist[4] == 0.0f;
    return NMI_OK;
}

extern "C" {

int nmi_undistort_frame(nmi_ctx *ctx, const double K[9], const float dist[5], const uint8_t *d_raw, const uint8_t *d_raw_mask, uint8_t *d_frame,
                        uint8_t *d_frame_mask)
{
    if (!ctx || !d_raw || !d_frame || d_raw == d_frame) return NMI_ERR_INVALID_ARGUMENT;
    if (d_frame_mask && (d_frame_mask == d_raw || d_frame_mask == d_frame || d_frame_mask == d_raw_mask)) return NMI_ERR_INVALID_ARGUMENT;
    if (d_raw_mask && d_raw_mask == d_frame) return NMI_ERR_INVALID_ARGUMENT;
    nmi::UndistortParams p;
    if (undistort_params(K, dist, &p, nullptr) != NMI_OK) return NMI_ERR_INVALID_ARGUMENT;
    ctx->detail.clear();
    DeviceGuard guard(ctx->device);
    NMI_HIP_TRY(ctx, nmi::launch_undistort(p, d_raw, d_raw_mask, d_frame, d_frame_mask, ctx->params.width, ctx->params.height, ctx->stream));
    return NMI_OK;
}

}  // extern "C"
