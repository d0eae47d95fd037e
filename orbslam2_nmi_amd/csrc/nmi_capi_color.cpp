// nmi_capi_color.cpp -- nmi_gray_frame (include/nmi_hip.h) and the host side of the frame formats the captured levels and streams
// share (nmi_level_set_frame_format, nmi_stream_set_frame_format: both through nmi_capi_intake.cpp's intake_set_frame and
// launch_intake).  Kernels: nmi_color.hip, nmi_bayer.hip (mosaics), and the colour instantiation of the undistortion kernel in
// nmi_undistort.hip; deep grey frames (GRAY16 and the formats that unpack to it) go through their tone table (nmi_tone.h).
#include "nmi_color.h"
#include "nmi_ctx.h"

using namespace nmi_internal;

int nmi_internal::frame_bytes_per_pixel(int32_t format)
{
    switch (format) {
    case NMI_FRAME_GRAY: return 1;
    case NMI_FRAME_BGR:
    case NMI_FRAME_RGB: return 3;
    case NMI_FRAME_BGRA:
    case NMI_FRAME_RGBA: return 4;
    case NMI_FRAME_YUYV:
    case NMI_FRAME_UYVY:
    case NMI_FRAME_GRAY16:
    case NMI_FRAME_GRAY16_BE:
    case NMI_FRAME_BAYER16_RGGB:
    case NMI_FRAME_BAYER16_GRBG:
    case NMI_FRAME_BAYER16_GBRG:
    case NMI_FRAME_BAYER16_BGGR: return 2;
    case NMI_FRAME_BAYER_RGGB:
    case NMI_FRAME_BAYER_GRBG:
    case NMI_FRAME_BAYER_GBRG:
    case NMI_FRAME_BAYER_BGGR: return 1;
    default: return 0;
    }
}

int64_t nmi_internal::frame_row_bytes(int32_t format, int64_t width)
{
    if (width <= 0) return 0;
    switch (format) {
    case NMI_FRAME_MONO10P:
    case NMI_FRAME_RAW10: return width % 4 == 0 ? width / 4 * 5 : 0;
    case NMI_FRAME_MONO12P:
    case NMI_FRAME_RAW12: return width % 2 == 0 ? width / 2 * 3 : 0;
    default: return width * frame_bytes_per_pixel(format);
    }
}

int nmi_internal::frame_format_check(int32_t format, int64_t pitch, int width, int height, int64_t *row_bytes, bool *identity)
{
    const int64_t dense = frame_row_bytes(format, width);
    if (dense == 0 || pitch < 0 || width <= 0 || height <= 0) return NMI_ERR_INVALID_ARGUMENT;
    // (the reflected edge needs a neighbour)
    if ((nmi::frame_is_bayer(format) || nmi::frame_is_bayer16(format)) && (width < 2 || height < 2)) return NMI_ERR_INVALID_ARGUMENT;
    if (nmi::frame_is_words(format) && (pitch % 2) != 0) return NMI_ERR_INVALID_ARGUMENT;
    if (nmi::frame_is_deep(format) && (int64_t)width * height > (int64_t)UINT32_MAX) return NMI_ERR_INVALID_ARGUMENT;
    if (pitch != 0 && pitch < dense) return NMI_ERR_INVALID_ARGUMENT;
    if (row_bytes) *row_bytes = pitch ? pitch : dense;
    if (identity) *identity = format == NMI_FRAME_GRAY && (pitch == 0 || pitch == dense);
    return NMI_OK;
}

int nmi_internal::frame_source_check(int32_t format, int64_t pitch, int32_t factor, int width, int height, const void *d_src, FrameSource *out)
{
    if (factor < 1 || factor > 4) return NMI_ERR_INVALID_ARGUMENT;
    const int64_t fW = (int64_t)factor * width, fH = (int64_t)factor * height;
    FrameSource s;
    if (fW > INT32_MAX || fH > INT32_MAX || frame_format_check(format, pitch, (int)fW, (int)fH, &s.row_bytes, &s.identity) != NMI_OK ||
        !frame_base_ok(format, d_src))
        return NMI_ERR_INVALID_ARGUMENT;
    s.width = (int)fW, s.height = (int)fH;
    s.bytes = span_of(d_src, (size_t)((fH - 1) * s.row_bytes + frame_row_bytes(format, fW)));
    *out = s;
    return NMI_OK;
}

extern "C" {

int nmi_gray_frame(nmi_ctx *ctx, const uint8_t *d_src, int32_t format, int64_t pitch, uint8_t *d_gray)
{
    if (!ctx || !d_src || !d_gray) return NMI_ERR_INVALID_ARGUMENT;
    const int W = ctx->params.width, H = ctx->params.height;
    FrameSource src;
    if (frame_source_check(format, pitch, 1, W, H, d_src, &src) != NMI_OK) return NMI_ERR_INVALID_ARGUMENT;
    const int64_t rb = src.row_bytes;
    if (meet(span_of(d_gray, ctx->npix), src.bytes)) return NMI_ERR_INVALID_ARGUMENT;  // the grey frame's H x W bytes
    ctx->detail.clear();
    DeviceGuard guard(ctx->device);
    if (nmi::frame_is_deep(format)) {  // through the context's tone map, as it is now (and through the container, if not GRAY16)
        const nmi::ToneSetting t = ctx->tone;
        NMI_HIP_TRY(ctx, tone_prepare(&ctx->tone_work, t, ctx->stream, container_bytes(format, 1, W, H)));
        NMI_HIP_TRY(ctx, deep_gray(ctx->tone_work, t, ctx->valid, d_src, format, rb, 1, nullptr, d_gray, nullptr, W, H, ctx->stream));
        return NMI_OK;
    }
    NMI_HIP_TRY(ctx, nmi::launch_gray(d_src, format, rb, d_gray, W, H, ctx->stream));
    return NMI_OK;
}

}  // extern "C"
