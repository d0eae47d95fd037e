// nmi_capi_undistort.cpp -- nmi_undistort_frame, nmi_undistort_frame_fisheye (include/nmi_hip.h) and the host side of the lens
// models the captured levels and streams share (nmi_level_set_distortion[_fisheye], nmi_stream_set_distortion[_fisheye]: all
// through nmi_capi_intake.cpp's intake_set_distortion[_fisheye] and launch_intake).  Kernel: nmi_undistort.hip.
#include "nmi_ctx.h"
#include "nmi_undistort.h"

using namespace nmi_internal;

namespace {

// K = [fx 0 cx; 0 fy cy; 0 0 1], finite, fx, fy > 0, also as fp32 -> its fp32 constants f = {fx, fy, cx, cy, 1/fx, 1/fy}.
bool camera_constants(const double K[9], float f[6])
{
    for (int i = 0; i < 9; ++i)
        if (!std::isfinite(K[i])) return false;
    // a pinhole camera without skew: [fx 0 cx; 0 fy cy; 0 0 1]
    if (K[1] != 0.0 || K[3] != 0.0 || K[6] != 0.0 || K[7] != 0.0 || K[8] != 1.0 || !(K[0] > 0.0) || !(K[4] > 0.0)) return false;
    f[0] = (float)K[0], f[1] = (float)K[4], f[2] = (float)K[2], f[3] = (float)K[5];
    f[4] = (float)(1.0 / K[0]), f[5] = (float)(1.0 / K[4]);
    for (int i = 0; i < 6; ++i)
        if (!std::isfinite(f[i])) return false;
    return f[0] > 0.0f && f[1] > 0.0f && f[4] > 0.0f && f[5] > 0.0f;  // (fl32 under- / overflow)
}

// The pointer rules nmi_undistort_frame and nmi_undistort_frame_fisheye share.
bool frame_pointers_ok(const nmi_ctx *ctx, const uint8_t *d_raw, const uint8_t *d_raw_mask, const uint8_t *d_frame, const uint8_t *d_frame_mask)
{
    if (!ctx || !d_raw || !d_frame || d_raw == d_frame) return false;
    if (d_frame_mask && (d_frame_mask == d_raw || d_frame_mask == d_frame || d_frame_mask == d_raw_mask)) return false;
    return !(d_raw_mask && d_raw_mask == d_frame);
}

}  // namespace

int nmi_internal::undistort_params(const double K[9], const float dist[5], nmi::UndistortParams *out, bool *identity)
{
    if (!K || !dist || !out) return NMI_ERR_INVALID_ARGUMENT;
    float f[6];
    if (!camera_constants(K, f)) return NMI_ERR_INVALID_ARGUMENT;
    for (int i = 0; i < 5; ++i)
        if (!std::isfinite(dist[i])) return NMI_ERR_INVALID_ARGUMENT;
    nmi::UndistortParams p{};
    p.model = nmi::kLensRadTan;
    p.fx = f[0], p.fy = f[1], p.cx = f[2], p.cy = f[3], p.ifx = f[4], p.ify = f[5];
    p.k1 = dist[0], p.k2 = dist[1], p.p1 = dist[2], p.p2 = dist[3], p.k3 = dist[4];
    *out = p;
    if (identity) *identity = dist[0] == 0.0f && dist[1] == 0.0f && dist[2] == 0.0f && dist[3] == 0.0f && dist[4] == 0.0f;
    return NMI_OK;
}

int nmi_internal::fisheye_params(const double K[9], const double K_raw[9], const float dist[4], nmi::UndistortParams *out)
{
    if (!K || !dist || !out) return NMI_ERR_INVALID_ARGUMENT;
    float f[6], fr[6];
    if (!camera_constants(K, f) || !camera_constants(K_raw ? K_raw : K, fr)) return NMI_ERR_INVALID_ARGUMENT;
    for (int i = 0; i < 4; ++i)
        if (!std::isfinite(dist[i])) return NMI_ERR_INVALID_ARGUMENT;
    nmi::UndistortParams p{};
    p.model = nmi::kLensFisheye;
    p.cxn = f[2], p.cyn = f[3], p.ifx = f[4], p.ify = f[5];
    p.fx = fr[0], p.fy = fr[1], p.cx = fr[2], p.cy = fr[3];
    p.k1 = dist[0], p.k2 = dist[1], p.k3 = dist[2], p.k4 = dist[3];
    *out = p;
    return NMI_OK;
}

extern "C" {

int nmi_undistort_frame(nmi_ctx *ctx, const double K[9], const float dist[5], const uint8_t *d_raw, const uint8_t *d_raw_mask, uint8_t *d_frame,
                        uint8_t *d_frame_mask)
{
    if (!frame_pointers_ok(ctx, d_raw, d_raw_mask, d_frame, d_frame_mask)) return NMI_ERR_INVALID_ARGUMENT;
    nmi::UndistortParams p;
    if (undistort_params(K, dist, &p, nullptr) != NMI_OK) return NMI_ERR_INVALID_ARGUMENT;
    ctx->detail.clear();
    DeviceGuard guard(ctx->device);
    NMI_HIP_TRY(ctx, nmi::launch_undistort(p, d_raw, d_raw_mask, d_frame, d_frame_mask, ctx->params.width, ctx->params.height, ctx->stream));
    return NMI_OK;
}

int nmi_undistort_frame_fisheye(nmi_ctx *ctx, const double K[9], const double K_raw[9], const float dist[4], const uint8_t *d_raw,
                                const uint8_t *d_raw_mask, uint8_t *d_frame, uint8_t *d_frame_mask)
{
    if (!frame_pointers_ok(ctx, d_raw, d_raw_mask, d_frame, d_frame_mask)) return NMI_ERR_INVALID_ARGUMENT;
    nmi::UndistortParams p;
    if (fisheye_params(K, K_raw, dist, &p) != NMI_OK) return NMI_ERR_INVALID_ARGUMENT;
    ctx->detail.clear();
    DeviceGuard guard(ctx->device);
    NMI_HIP_TRY(ctx, nmi::launch_undistort(p, d_raw, d_raw_mask, d_frame, d_frame_mask, ctx->params.width, ctx->params.height, ctx->stream));
    return NMI_OK;
}

}  // extern "C"
