// nmi_capi_masked.cpp -- the masked entry points of include/nmi_hip.h: nmi_warp_stack_masked, nmi_search_grid_masked,
// nmi_last_mask_counts; and what the masked and covered searches share on the host: their kernel arguments, their launches and
// their enqueue (nmi_capi_covered.cpp, the levels and the streams of nmi_capi_pipeline.cpp use them).  Kernels:
// nmi_masked_producer.hip, nmi_masked_kernel.hip, nmi_masked_pix_kernel.hip (mid-size grids).
#include "nmi_ctx.h"

using namespace nmi_internal;

namespace {

// Counts and tables for Wn warps.  Growing waits for the stream (the old buffers may be in use by a search in flight).
int ensure_mask_work(nmi_ctx *ctx, int Wn)
{
    if (Wn > ctx->mask_warps_cap) {
        NMI_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        if (ctx->d_mask_counts) NMI_HIP_TRY(ctx, hipFree(ctx->d_mask_counts));
        if (ctx->d_mask_tables) NMI_HIP_TRY(ctx, hipFree(ctx->d_mask_tables));
        ctx->d_mask_counts = nullptr;
        ctx->d_mask_tables = nullptr;
        ctx->mask_warps_cap = 0;
        ctx->mask_count_n = 0;
        NMI_HIP_TRY(ctx, hipMalloc((void **)&ctx->d_mask_counts, (size_t)Wn * sizeof(int32_t)));
        NMI_HIP_TRY(ctx, hipMalloc((void **)&ctx->d_mask_tables, (size_t)Wn * ((size_t)ctx->npix + 1) * sizeof(float)));
        ctx->mask_warps_cap = Wn;
    }
    return NMI_OK;
}

}  // namespace

// The redo list of `total` candidates.  Growing waits for the stream (the old list may be in use by a search in flight).
int nmi_internal::ensure_mask_redo(nmi_ctx *ctx, int64_t total)
{
    if (!ctx->d_mask_redo_state) {
        NMI_HIP_TRY(ctx, hipMalloc((void **)&ctx->d_mask_redo_state, 2 * sizeof(uint32_t)));
        NMI_HIP_TRY(ctx, hipMemsetAsync(ctx->d_mask_redo_state, 0, 2 * sizeof(uint32_t), ctx->stream));
    }
    if (total > ctx->mask_redo_cap) {
        NMI_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        if (ctx->d_mask_redo) NMI_HIP_TRY(ctx, hipFree(ctx->d_mask_redo));
        ctx->d_mask_redo = nullptr;
        ctx->mask_redo_cap = 0;
        NMI_HIP_TRY(ctx, hipMalloc((void **)&ctx->d_mask_redo, (size_t)total * sizeof(int32_t)));
        ctx->mask_redo_cap = total;
    }
    return NMI_OK;
}

MaskSearch nmi_internal::mask_search_args(const nmi::GridArgs &a, const uint8_t *warp_masks, const uint8_t *render_masks, int32_t *counts,
                                          const float *tables, int32_t *redo, uint32_t *redo_state)
{
    MaskSearch ms{};
    ms.covered = render_masks != nullptr;
    if (ms.covered) {
        nmi::CoveredGridArgs &m = ms.cover;
        m.g = a;
        m.warp_masks = warp_masks;
        m.render_masks = render_masks;
        m.counts = counts;
        m.vec_ok = a.vec_ok && (((uintptr_t)warp_masks | (uintptr_t)render_masks) % 16) == 0;
        m.redo = redo;
        m.redo_n = redo_state;
        m.redo_done = redo_state + 1;
    } else {
        nmi::MaskedGridArgs &m = ms.masked;
        m.g = a;
        m.warp_masks = warp_masks;
        m.tables = tables;
        m.counts = counts;
        m.vec_ok = a.vec_ok && ((uintptr_t)warp_masks % 16) == 0;
        m.redo = redo;
        m.redo_n = redo_state;
        m.redo_done = redo_state + 1;
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
// covered stream tickets): the covered search when render_masks is set, see mask_search_args.  out_key: optional device word
// that receives the packed key; post: the caller polls the mailbox (the blocking call).  Commits enqueue_grid's protocol
// bookkeeping once the launches are accepted.  S_local * Wn > 0.
int nmi_internal::enqueue_grid_mask(nmi_ctx *ctx, const uint8_t *render_stack, const uint8_t *render_masks, int S_local, int s_offset,
                                    int S_total, const uint8_t *warp_stack, const uint8_t *warp_masks, int Wn, int w_offset, int32_t *counts,
                                    const float *tables, int32_t *redo, uint32_t *redo_state, float *d_ratings, unsigned long long *out_key,
                                    bool post)
{
    const nmi_params &p = ctx->params;
    const int64_t total = (int64_t)S_local * Wn;
    int rc = NMI_OK;
    nmi::GridArgs a{};
    a.render_stack = render_stack;
    a.warp_stack = warp_stack;
    a.S_local = S_local;
    a.Wn = Wn;
    a.s_offset = s_offset;
    a.S_total = S_total;
    a.w_offset = w_offset;
    nmi::set_geometry(a, p.width, p.height, render_stack, warp_stack, p.render_bottom_up != 0);
    a.shift = ctx->shift;
    a.mode = p.mode;
    a.table = nullptr;
    a.plan = nullptr;
    a.ratings = d_ratings;
    a.key = ctx->d_keys + ctx->slot;
    a.reset_key = ctx->d_keys + (ctx->slot ^ 1);
    a.out_key = out_key;
    a.done = ctx->d_done;
    post = post && ctx->result_path == 1;
    a.mailbox = post ? ctx->mailbox : nullptr;
    a.seq = post ? ctx->seq + 1 : 0;
    a.hist_variant = ctx->hist_variant;
    a.phase_mask = 3;
    const int cap = ctx->workgroups > 0 ? ctx->workgroups : ctx->compute_units;
    const int workgroups = (int)(total < cap ? total : cap);
    // mid-size grids: pixel ranges (nmi_masked_pix_kernel.hip, nmi_covered_pix_kernel.hip), by nmi_search_grid's rules and
    // controls (choose_pix)
    const int pix = choose_pix(ctx, a, total, cap);
    if (pix) {
        rc = ensure_pix_blocks(ctx, nmi::pix_block_bytes((int)total, pix));
        if (rc == NMI_OK) rc = next_split_epoch(ctx, &a.epoch);
        if (rc == NMI_OK) rc = ensure_pix_timeouts(ctx);
        if (rc != NMI_OK) return rc;
        a.blocks = ctx->d_pix_blocks;
        a.phase_mask = 3 | (ctx->phase_mask & 512);  // (bit 9: the helpers' hand-off test hook, as for nmi_pix_kernel)
    } else if (ctx->xcd_tiling && total <= (1ll << 24)) {
        rc = ensure_order(ctx, S_local, Wn, &a.order);
        if (rc != NMI_OK) return rc;
    }
    const MaskSearch ms = mask_search_args(a, warp_masks, render_masks, counts, tables, redo, redo_state);
    // timed (nmi_set_profiling): the scoring launches, as for nmi_search_grid -- not the masked search's counts and tables before them
    if (ctx->profiling) NMI_HIP_TRY(ctx, hipEventRecord(ctx->ev_start, ctx->stream));
    NMI_HIP_TRY(ctx, launch_mask_search(ms, pix, pix ? pix_owner_share(ctx, pix) : 0.0, workgroups, p.use_bg != 0, ctx->hist_variant == 1, nullptr,
                                        ctx->d_pix_timeouts, ctx->stream));
    // accepted: commit the protocol state (enqueue_grid's bookkeeping)
    if (post) ++ctx->seq;
    ctx->posted = post;
    ctx->last_slot = ctx->slot;
    ctx->slot ^= 1;
    ctx->last_parts = 0;
    ctx->last_pix = pix;
    ctx->last_epoch = 0;
    ctx->last_few = 0;
    if (ctx->profiling) {
        NMI_HIP_TRY(ctx, hipEventRecord(ctx->ev_stop, ctx->stream));
        ctx->have_timing = true;
    }
    return NMI_OK;
}

extern "C" {

int nmi_warp_stack_masked(nmi_ctx *ctx, const uint8_t *d_frame, const uint8_t *d_frame_mask, const double *h_forward, int32_t Wn,
                          uint8_t *d_warp_stack, uint8_t *d_warp_masks)
{
    if (!ctx || !d_frame || !h_forward || !d_warp_stack || !d_warp_masks || Wn <= 0) return NMI_ERR_INVALID_ARGUMENT;
    // the warps themselves: nmi_warp_stack, byte for byte (it uploads the inverse maps to a ring slot of the context)
    int rc = nmi_warp_stack(ctx, d_frame, h_forward, Wn, d_warp_stack);
    if (rc != NMI_OK) return rc;
    DeviceGuard guard(ctx->device);
    const int ring = (int)((ctx->warp_uses - 1) % nmi_ctx::kWarpRing);  // the slot nmi_warp_stack just used
    NMI_HIP_TRY(ctx, nmi::launch_warp_masks(d_frame_mask, ctx->d_warp_coeffs[ring], d_warp_masks, ctx->params.width, ctx->params.height,
                                            Wn, ctx->stream));
    NMI_HIP_TRY(ctx, hipEventRecord(ctx->warp_ev[ring], ctx->stream));  // the slot is free again after this kernel too
    return NMI_OK;
}

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
        NMI_HIP_TRY(ctx, nmi::launch_mask_counts(warp_masks, Wn, ctx->npix, ctx->d_mask_counts, ctx->stream));
        NMI_HIP_TRY(ctx, nmi::launch_mask_tables(ctx->d_mask_counts, Wn, ctx->npix, ctx->d_mask_tables, ctx->stream));
        ctx->mask_count_n = Wn;
    }
    if (total == 0) {  // nothing to score: no winner (as nmi_search_grid)
        NMI_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        ctx->have_timing = false;
        return nmi_key_unpack(0, h_best_index, h_best_score);
    }

    rc = enqueue_grid_mask(ctx, render_stack, nullptr, S, 0, S, warp_stack, warp_masks, Wn, 0, ctx->d_mask_counts, ctx->d_mask_tables,
                           ctx->d_mask_redo, ctx->d_mask_redo_state, d_ratings, nullptr, /*post=*/true);
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
    NMI_HIP_TRY(ctx, hipMemcpyAsync(h_counts, ctx->d_mask_counts, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    NMI_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return NMI_OK;
}

}  // extern "C"
