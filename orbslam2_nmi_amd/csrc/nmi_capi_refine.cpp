// nmi_capi_refine.cpp -- C ABI of the refined peaks of a rating table (include/nmi_hip.h, "Refined peaks"): nmi_refine_peaks.  The
// level form (nmi_level_set_refine, nmi_level_copy_refined) is with the other level setters in nmi_capi_pipeline.cpp.
#include "nmi_ctx.h"
#include "nmi_refine.h"

using namespace nmi_internal;

extern "C" {

int nmi_refine_peaks(nmi_ctx *ctx, const float *d_ratings, const int32_t num[6], const uint64_t *d_keys, const uint64_t *h_keys, int32_t K,
                     nmi_refined_peak *d_out, nmi_refined_peak *h_out)
{
    if (!ctx || !d_ratings || !num || K < 1 || K > nmi::kRefineMaxK || (d_keys != nullptr) == (h_keys != nullptr) || (!d_out && !h_out))
        return NMI_ERR_INVALID_ARGUMENT;
    const int64_t cells = nmi::refine_cells(num);
    if (cells == 0) return NMI_ERR_INVALID_ARGUMENT;
    if (cells < 0) return NMI_ERR_UNSUPPORTED;  // the index lives in 32 bits of the key
    ctx->detail.clear();
    DeviceGuard guard(ctx->device);
    nmi::RefineArgs a;
    a.ratings = d_ratings;
    for (int i = 0; i < 6; ++i) a.num[i] = num[i];
    a.cells = (uint32_t)cells;
    a.K = K;
    a.keys = (const unsigned long long *)d_keys;
    if (h_keys)
        for (int k = 0; k < K; ++k) a.host_keys[k] = h_keys[k];
    a.out = d_out;
    constexpr size_t kRecords = nmi::kRefineMaxK * sizeof(nmi_refined_peak);
    if (h_out) {  // the kernel writes the records to mapped host memory and posts the call's number behind each
        if (!ctx->h_refine) {
            NMI_HIP_TRY(ctx, ctx->h_refine.alloc(kRecords + nmi::kRefineMaxK * sizeof(unsigned long long), nmi_mem::kPosted));
            memset(ctx->h_refine.as<>(), 0, ctx->h_refine.size());  // (no call has number 0)
        }
        a.out_host = ctx->h_refine.device<nmi_refined_peak>();
        a.post = (unsigned long long *)((char *)ctx->h_refine.device<>() + kRecords);
        a.seq = ++ctx->refine_seq;
    }
    NMI_HIP_TRY(ctx, nmi::launch_refine(a, ctx->stream));
    if (!h_out) return NMI_OK;
    // One polled word per record (as nmi_rank_peaks polls its one): the K workgroups end within a few hundred nanoseconds of each
    // other.  A stream that drained without a post cannot happen with a kernel that ran; the records are then read after the drain.
    const volatile unsigned long long *posted = (const volatile unsigned long long *)((char *)ctx->h_refine.as<>() + kRecords);
    bool drained = false;
    for (int k = 0; k < K && !drained; ++k) {
        unsigned long long word = 0;
        const int rc = wait_word(ctx, posted + k, ~0ull, a.seq, &word);
        if (rc != NMI_OK && rc != NMI_ERR_NOT_READY) return rc;
        drained = rc == NMI_ERR_NOT_READY;
    }
    if (drained || d_out) NMI_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // d_out: readable from any stream on return
    memcpy(h_out, ctx->h_refine.as<>(), (size_t)K * sizeof(nmi_refined_peak));
    return NMI_OK;
}

}  // extern "C"
