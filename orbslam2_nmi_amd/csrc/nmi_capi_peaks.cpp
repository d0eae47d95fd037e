// nmi_capi_peaks.cpp -- C ABI of the ranked peaks of a rating table (include/nmi_hip.h, "Ranked peaks"): nmi_rank_peaks.  The
// level form (nmi_level_set_peaks, nmi_level_copy_peaks) is with the other level setters in nmi_capi_pipeline.cpp.
#include "nmi_ctx.h"
#include "nmi_peaks.h"

using namespace nmi_internal;

extern "C" {

int nmi_rank_peaks(nmi_ctx *ctx, const float *d_ratings, const int32_t num[6], int32_t K, const int32_t radius[6], uint64_t *d_keys,
                   uint64_t *h_keys, int32_t *h_count)
{
    if (!ctx || !d_ratings || !num || !radius || K < 1 || K > nmi::kPeaksMaxK || (!d_keys && !h_keys)) return NMI_ERR_INVALID_ARGUMENT;
    nmi::PeaksArgs a;
    const int shape = nmi::peaks_shape(num, radius, a);
    if (shape != 0) return shape == -1 ? NMI_ERR_INVALID_ARGUMENT : NMI_ERR_UNSUPPORTED;
    ctx->detail.clear();
    DeviceGuard guard(ctx->device);
    a.ratings = d_ratings;
    a.K = K;
    a.out = (unsigned long long *)d_keys;
    if (h_keys) {  // the kernel writes the keys to mapped host memory and posts the call's number behind them
        if (!ctx->h_peaks) {
            NMI_HIP_TRY(ctx, ctx->h_peaks.alloc((nmi::kPeaksMaxK + 1) * sizeof(unsigned long long), nmi_mem::kPosted));
            memset(ctx->h_peaks.as<>(), 0, ctx->h_peaks.size());  // (no call has number 0)
        }
        a.out_host = ctx->h_peaks.device<unsigned long long>();
        a.post = a.out_host + nmi::kPeaksMaxK;
        a.seq = ++ctx->peaks_seq;
    }
    NMI_HIP_TRY(ctx, nmi::launch_peaks(a, ctx->stream));
    if (!h_keys) return NMI_OK;
    // Polling the posted word returns earlier than waiting for the stream to drain (as fetch_key does for the search's winner).  A
    // stream that drained without the post cannot happen with a kernel that ran; the keys are then read after the drain anyway.
    unsigned long long word = 0;
    const int rc = wait_word(ctx, ctx->h_peaks.as<unsigned long long>() + nmi::kPeaksMaxK, ~0ull, a.seq, &word);
    if (rc != NMI_OK && rc != NMI_ERR_NOT_READY) return rc;
    if (rc == NMI_ERR_NOT_READY || d_keys) NMI_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // d_keys: readable from any stream on return
    memcpy(h_keys, ctx->h_peaks.as<>(), (size_t)K * sizeof(uint64_t));
    if (h_count) {
        int32_t n = 0;
        while (n < K && h_keys[n] != 0) ++n;  // (zeros follow the peaks: none in between)
        *h_count = n;
    }
    return NMI_OK;
}

}  // extern "C"
