// nmi_capi_reduce.cpp -- nmi_reduce_frame (include/nmi_hip.h): a full-size camera frame to the grey frame of the search size.
// The captured levels and streams use the same kernels (nmi_level_set_frame_reduction, nmi_stream_set_frame_reduction: both
// through nmi_capi_intake.cpp's intake_set_frame and launch_intake).  Kernels: nmi_reduce.hip; factor 1 is nmi_color.hip's
// conversion.
#include "nmi_color.h"
#include "nmi_ctx.h"
#include "nmi_reduce.h"

using namespace nmi_internal;

namespace {

struct Span {
    uintptr_t lo, hi;  // [lo, hi); lo == hi: nothing
};

bool meet(const Span &a, const Span &b) { return a.lo < a.hi && b.lo < b.hi && a.lo < b.hi && b.lo < a.hi; }

}  // namespace

extern "C" {

int nmi_reduce_frame(nmi_ctx *ctx, const uint8_t *d_src, int32_t format, int64_t pitch, int32_t factor, const uint8_t *d_src_mask,
                     uint8_t *d_gray, uint8_t *d_mask)
{
    if (!ctx || !d_src || !d_gray) return NMI_ERR_INVALID_ARGUMENT;
    if (factor < 1 || factor > 4) return NMI_ERR_INVALID_ARGUMENT;
    if ((d_src_mask == nullptr) != (d_mask == nullptr)) return NMI_ERR_INVALID_ARGUMENT;
    const int W = ctx->params.width, H = ctx->params.height;
    const int64_t fW = (int64_t)factor * W, fH = (int64_t)factor * H;
    if (fW > INT32_MAX || fH > INT32_MAX) return NMI_ERR_INVALID_ARGUMENT;
    int64_t rb = 0;
    if (frame_format_check(format, pitch, (int)fW, (int)fH, &rb, nullptr) != NMI_OK || !frame_base_ok(format, d_src)) return NMI_ERR_INVALID_ARGUMENT;
    // the source's bytes run from d_src to the end of its last row's pixels, the source mask's over its dense f H x f W bytes;
    // neither output may meet them, or the other output
    const uintptr_t s0 = (uintptr_t)d_src, m0 = (uintptr_t)d_src_mask, g0 = (uintptr_t)d_gray, o0 = (uintptr_t)d_mask;
    const Span src{s0, s0 + (uintptr_t)((fH - 1) * rb + frame_row_bytes(format, fW))};
    const Span src_mask{m0, d_src_mask ? m0 + (uintptr_t)(fW * fH) : m0};
    const Span gray{g0, g0 + (uintptr_t)ctx->npix};
    const Span mask{o0, d_mask ? o0 + (uintptr_t)ctx->npix : o0};
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
