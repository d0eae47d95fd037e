// nmi_capi_reduce.cpp -- nmi_reduce_frame (include/nmi_hip.h): a full-size camera frame to the grey frame of the search size.
// The captured levels and streams use the same kernels (nmi_level_set_frame_reduction, nmi_stream_set_frame_reduction: both
// through nmi_capi_intake.cpp's intake_set_frame and launch_intake).  Kernels: nmi_reduce.hip; factor 1 is nmi_color.hip's
// conversion.
#include "nmi_color.h"
#include "nmi_ctx.h"
#include "nmi_reduce.h"

using namespace nmi_internal;

extern "C" {

int nmi_reduce_frame(nmi_ctx *ctx, const uint8_t *d_src, int32_t format, int64_t pitch, int32_t factor, const uint8_t *d_src_mask,
                     uint8_t *d_gray, uint8_t *d_mask)
{
    if (!ctx || !d_src || !d_gray) return NMI_ERR_INVALID_ARGUMENT;
    if ((d_src_mask == nullptr) != (d_mask == nullptr)) return NMI_ERR_INVALID_ARGUMENT;
    const int W = ctx->params.width, H = ctx->params.height;
    FrameSource full;
    if (frame_source_check(format, pitch, factor, W, H, d_src, &full) != NMI_OK) return NMI_ERR_INVALID_ARGUMENT;
    const int64_t rb = full.row_bytes;
    // the source mask's bytes are its dense f H x f W; neither output may meet the source's or the source mask's, or the other output
    const Span src = full.bytes, src_mask = span_of(d_src_mask, (size_t)full.width * full.height);
    const Span gray = span_of(d_gray, ctx->npix), mask = span_of(d_mask, ctx->npix);
    if (meet(gray, src) || meet(gray, src_mask) || meet(mask, src) || meet(mask, src_mask) || meet(gray, mask)) return NMI_ERR_INVALID_ARGUMENT;
    ctx->detail.clear();
    DeviceGuard guard(ctx->device);
    if (nmi::frame_is_deep(format)) {  // the tone table from the full-size frame, then nmi_tone.hip's conversion at every factor
        const nmi::ToneSetting t = ctx->tone;
        NMI_HIP_TRY(ctx, tone_prepare(&ctx->tone_work, t, ctx->stream, container_bytes(format, factor, W, H)));
        const nmi::ValidRange range = ctx->valid;
        if (d_mask && range.on()) {  // the mask pair's rule first, then validity ANDed into it by the conversion (in place)
            NMI_HIP_TRY(ctx, nmi::launch_reduce_mask(d_src_mask, factor, d_mask, W, H, ctx->stream));
            NMI_HIP_TRY(ctx, deep_gray(ctx->tone_work, t, range, d_src, format, rb, factor, d_mask, d_gray, d_mask, W, H, ctx->stream));
            return NMI_OK;
        }
        NMI_HIP_TRY(ctx, deep_gray(ctx->tone_work, t, range, d_src, format, rb, factor, nullptr, d_gray, nullptr, W, H, ctx->stream));
    } else if (factor == 1) {  // nmi_gray_frame; the mask is copied as 0 / 1
        NMI_HIP_TRY(ctx, nmi::launch_gray(d_src, format, rb, d_gray, W, H, ctx->stream));
    } else {
        NMI_HIP_TRY(ctx, nmi::launch_reduce(d_src, format, rb, factor, d_gray, W, H, ctx->stream));
    }
    if (d_mask) NMI_HIP_TRY(ctx, nmi::launch_reduce_mask(d_src_mask, factor, d_mask, W, H, ctx->stream));
    return NMI_OK;
}

}  // extern "C"
