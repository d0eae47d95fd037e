// nmi_capi_masked.cpp -- the masked entry points of include/nmi_hip.h: nmi_search_grid_masked (nmi_warp_stack_masked is beside nmi_warp_stack),
// nmi_last_mask_counts; and what the masked and covered searches share on the host: their kernel arguments, their launches and
// their enqueue (nmi_capi_covered.cpp, the levels and the streams of nmi_capi_pipeline.cpp use them).  Kernels:
// nmi_masked_producer.hip, nmi_masked_kernel.hip, nmi_masked_pix_kernel.hip (mid-size grids).
#include "nmi_ctx.h"

using namespace nmi_internal;

namespace {

// Counts and tables for Wn warps.  Growing waits for the stream (the old buffers may be in use by a search in flight).
int ensure_mask_work(nmi_ctx *ctx, int Wn)
{
    if ((size_t)Wn * sizeof(int32_t) > ctx->d_mask_counts.size()) ctx->mask_count_n = 0;
    NMI_HIP_TRY(ctx, ctx->d_mask_counts.grow((size_t)Wn * sizeof(int32_t), ctx->stream));
    NMI_HIP_TRY(ctx, ctx->d_mask_tables.grow((size_t)Wn * ((size_t)ctx->npix + 1) * sizeof(float), ctx->stream));
    return NMI_OK;
}

}  // namespace

// The redo list of `total` candidates.  Growing waits for the stream (the old list may be in use by a search in flight).
int nmi_internal::ensure_mask_redo(nmi_ctx *ctx, int64_t total)
{
    NMI_HIP_TRY(ctx, ctx->d_mask_redo_state.grow(2 * sizeof(uint32_t), ctx->stream, /*zero=*/true));
    NMI_HIP_TRY(ctx, ctx->d_mask_redo.grow((size_t)total * sizeof(int32_t), ctx->stream));
    return NMI_OK;
}

MaskSearch nmi_internal::mask_search_args(const nmi::GridArgs &a, const MaskSide &side)
{
    MaskSearch ms{};
    ms.covered = side.render_masks != nullptr;
    if (ms.covered) {
        nmi::CoveredGridArgs &m = ms.cover;
        m.g = a;
        m.warp_masks = side.warp_masks;
        m.render_masks = side.render_masks;
        m.counts = side.counts;
        m.vec_ok = a.vec_ok && (((uintptr_t)side.warp_masks | (uintptr_t)side.render_masks) % 16) == 0;
        m.redo = side.redo;
        m.redo_n = side.redo_state;
        m.redo_done = side.redo_state + 1;
    } else {
        nmi::MaskedGridArgs &m = ms.masked;
        m.g = a;
        m.warp_masks = side.warp_masks;
        m.tables = side.tables;
        m.counts = side.counts;
        m.vec_ok = a.vec_ok && ((uintptr_t)side.warp_masks % 16) == 0;
        m.redo = side.redo;
        m.redo_n = side.redo_state;
        m.redo_done = side.redo_state + 1;
    }
    return ms;
}

hipError_t nmi_internal::launch_mask_search(const MaskSearch &ms, int pix, double owner_share, int workgroups, bool use_bg, bool exact,
                                            const uint32_t *replay, uint32_t *healed, hipStream_t stream)
{
    if (ms.covered)
        return pix ? nmi::launch_pix_covered(ms.cover, pix, owner_share, use_bg, replay, healed, stream)
                   : nmi::launch_grid_covered(ms.cover, workgroups, use_bg, exact, stream);
    return pix ? nmi::launch_pix_masked(ms.masked, pix, owner_share, use_bg, replay, healed, stream)
               : nmi::launch_grid_masked(ms.masked, workgroups, use_bg, exact, stream);
}

// nmi_search_grid_masked's and nmi_search_grid_covered's launches without their blocking tails (they also serve the masked and
// covered stream tickets): the covered search when m.render_masks is set, see MaskSide.  enqueue_grid's steps and its protocol
// bookkeeping (commit_launch).  S_local * Wn > 0.
int nmi_internal::enqueue_grid_mask(nmi_ctx *ctx, const SearchRequest &rq, const MaskSide &m, SearchLaunch *launched)
{
    const nmi_params &p = ctx->params;
    const bool post = rq.post && ctx->result_path == 1;
    nmi::GridArgs a = grid_args(ctx, rq, post, false);  // (no term table, no probe's plan: MaskSearch)
    // mid-size grids: pixel ranges (nmi_masked_pix_kernel.hip, nmi_covered_pix_kernel.hip), by nmi_search_grid's rules and controls
    const nmi::SearchPlan plan = nmi::plan_search(plan_inputs(ctx, nmi::SearchForm::masked, (int64_t)rq.S_local * rq.Wn, a));
    a.phase_mask = plan.phase_mask;
    const int rc = prepare_search(ctx, plan, a);
    if (rc != NMI_OK) return rc;
    const MaskSearch ms = mask_search_args(a, m);
    // timed (nmi_set_profiling): the scoring launches, as for nmi_search_grid -- not the masked search's counts and tables before them
    if (ctx->profiling) NMI_HIP_TRY(ctx, hipEventRecord(ctx->ev_start, ctx->stream));
    NMI_HIP_TRY(ctx, launch_mask_search(ms, plan.pix, plan.pix ? pix_owner_share(ctx, plan.pix) : 0.0, plan.workgroups, p.use_bg != 0,
                                        ctx->hist_variant == 1, nullptr, ctx->d_pix_timeouts.as<uint32_t>(), ctx->stream));
    return commit_launch(ctx, post, false, SearchLaunch{plan.kind, 0, plan.pix, 0, 0}, /*launched=*/true, launched);
}

extern "C" {

int nmi_search_grid_masked(nmi_ctx *ctx, const uint8_t *render_stack, int32_t S, const uint8_t *warp_stack, const uint8_t *warp_masks,
                           int32_t Wn, float *d_ratings, int64_t *h_best_index, float *h_best_score)
{
    int rc = check_grid_args(ctx, render_stack, S, 0, S, warp_stack, Wn);
    if (rc != NMI_OK) return rc;
    if (!warp_masks) return NMI_ERR_INVALID_ARGUMENT;  // never the unmasked search in disguise
    DeviceGuard guard(ctx->device);
    const int64_t total = (int64_t)S * Wn;
    if (Wn > 0) {
        rc = ensure_mask_work(ctx, Wn);
        if (rc == NMI_OK) rc = ensure_mask_redo(ctx, total);
        if (rc != NMI_OK) return rc;
        // len_w from the masks of THIS call (they need not come from nmi_warp_stack_masked), then the per-warp tables
        NMI_HIP_TRY(ctx, nmi::launch_mask_counts(warp_masks, Wn, ctx->npix, ctx->d_mask_counts.as<int32_t>(), ctx->stream));
        NMI_HIP_TRY(ctx, nmi::launch_mask_tables(ctx->d_mask_counts.as<int32_t>(), Wn, ctx->npix, ctx->d_mask_tables.as<float>(), ctx->stream));
        ctx->mask_count_n = Wn;
    }
    if (total == 0) {  // nothing to score: no winner (as nmi_search_grid)
        NMI_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        ctx->have_timing = false;
        return nmi_key_unpack(0, h_best_index, h_best_score);
    }

    SearchRequest rq = SearchRequest::block(render_stack, S, 0, S, warp_stack, Wn);
    rq.d_ratings = d_ratings;
    rq.post = true;
    rc = enqueue_grid_mask(ctx, rq, MaskSide{warp_masks, nullptr, ctx->d_mask_counts.as<int32_t>(), ctx->d_mask_tables.as<float>(), ctx->d_mask_redo.as<int32_t>(),
                                                ctx->d_mask_redo_state.as<uint32_t>()});
    if (rc != NMI_OK) return rc;
    unsigned long long key = 0;
    rc = fetch_key(ctx, &key);
    if (rc != NMI_OK) return rc;
    // the rating table must be complete and visible to every stream when the call returns (as nmi_search_grid)
    if (d_ratings) NMI_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return nmi_key_unpack(key, h_best_index, h_best_score);
}

int nmi_last_mask_counts(nmi_ctx *ctx, int32_t *h_counts, int32_t n)
{
    if (!ctx || !h_counts || n < 0 || n > ctx->mask_count_n) return NMI_ERR_INVALID_ARGUMENT;
    if (n == 0) return NMI_OK;
    DeviceGuard guard(ctx->device);
    NMI_HIP_TRY(ctx, hipMemcpyAsync(h_counts, ctx->d_mask_counts.as<>(), (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    NMI_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return NMI_OK;
}

}  // extern "C"
