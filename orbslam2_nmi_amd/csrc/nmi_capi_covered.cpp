// nmi_capi_covered.cpp -- the covered entry points of include/nmi_hip.h: nmi_search_grid_covered, nmi_last_cover_counts,
// nmi_render_points_masked, nmi_render_mesh_masked.  Kernels: nmi_covered_kernel.hip and nmi_covered_pix_kernel.hip (mid-size
// grids) for the search, nmi_producers.hip and nmi_mesh.hip (the coverage forms of the renderers' last pass); and
// nmi_pack_mask_bits (nmi_mask_bits.hip), which packs such coverage into the bits a covered stream ticket carries.
#include "nmi_covered.h"
#include "nmi_ctx.h"
#include "nmi_mask_bits.h"

using namespace nmi_internal;

namespace {

// Counts [total] and the redo list of `total` candidates.  Growing waits for the stream (the old buffers may be in use by a
// search in flight).
int ensure_cover_work(nmi_ctx *ctx, int64_t total)
{
    if (!ctx->d_cover_redo_state) {
        NMI_HIP_TRY(ctx, hipMalloc((void **)&ctx->d_cover_redo_state, 2 * sizeof(uint32_t)));
        NMI_HIP_TRY(ctx, hipMemsetAsync(ctx->d_cover_redo_state, 0, 2 * sizeof(uint32_t), ctx->stream));
    }
    if (total > ctx->cover_cap) {
        NMI_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        if (ctx->d_cover_counts) NMI_HIP_TRY(ctx, hipFree(ctx->d_cover_counts));
        if (ctx->d_cover_redo) NMI_HIP_TRY(ctx, hipFree(ctx->d_cover_redo));
        ctx->d_cover_counts = nullptr;
        ctx->d_cover_redo = nullptr;
        ctx->cover_cap = 0;
        ctx->cover_count_n = 0;
        NMI_HIP_TRY(ctx, hipMalloc((void **)&ctx->d_cover_counts, (size_t)total * sizeof(int32_t)));
        NMI_HIP_TRY(ctx, hipMalloc((void **)&ctx->d_cover_redo, (size_t)total * sizeof(int32_t)));
        ctx->cover_cap = total;
    }
    return NMI_OK;
}

}  // namespace

// nmi_search_grid_covered's launches without its blocking tail (it also serves covered stream tickets).  counts receives
// len[w][s] ([Wn][S_local]); redo has room for S_local * Wn candidates and redo_state [2] is zero.  out_key: optional device
// word that receives the packed key; post: the caller polls the mailbox (the blocking call).  Commits enqueue_grid's protocol
// bookkeeping once the launches are accepted.  S_local * Wn > 0.
int nmi_internal::enqueue_grid_covered(nmi_ctx *ctx, const uint8_t *render_stack, const uint8_t *render_masks, int S_local, int s_offset,
                                       int S_total, const uint8_t *warp_stack, const uint8_t *warp_masks, int Wn, int w_offset, int32_t *counts,
                                       int32_t *redo, uint32_t *redo_state, float *d_ratings, unsigned long long *out_key, bool post)
{
    const nmi_params &p = ctx->params;
    const int64_t total = (int64_t)S_local * Wn;
    int rc = NMI_OK;
    nmi::CoveredGridArgs m{};
    nmi::GridArgs &a = m.g;
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
    m.warp_masks = warp_masks;
    m.render_masks = render_masks;
    m.counts = counts;
    m.vec_ok = a.vec_ok && ((uintptr_t)warp_masks % 16) == 0 && ((uintptr_t)render_masks % 16) == 0;
    m.redo = redo;
    m.redo_n = redo_state;
    m.redo_done = redo_state + 1;
    const int cap = ctx->workgroups > 0 ? ctx->workgroups : ctx->compute_units;
    const int workgroups = (int)(total < cap ? total : cap);
    // mid-size grids: pixel ranges (nmi_covered_pix_kernel.hip), by nmi_search_grid's rules and controls (choose_pix)
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
    // timed (nmi_set_profiling): the scoring launches, as for nmi_search_grid
    if (ctx->profiling) NMI_HIP_TRY(ctx, hipEventRecord(ctx->ev_start, ctx->stream));
    if (pix)
        NMI_HIP_TRY(ctx, nmi::launch_pix_covered(m, pix, pix_owner_share(ctx, pix), p.use_bg != 0, nullptr, ctx->d_pix_timeouts, ctx->stream));
    else
        NMI_HIP_TRY(ctx, nmi::launch_grid_covered(m, workgroups, p.use_bg != 0, ctx->hist_variant == 1, ctx->stream));
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

int nmi_search_grid_covered(nmi_ctx *ctx, const uint8_t *render_stack, const uint8_t *render_masks, int32_t S, const uint8_t *warp_stack,
                            const uint8_t *warp_masks, int32_t Wn, float *d_ratings, int64_t *h_best_index, float *h_best_score)
{
    if (!ctx || !render_masks || !warp_masks || S < 1 || Wn < 1) return NMI_ERR_INVALID_ARGUMENT;
    int rc = check_grid_args(ctx, render_stack, S, 0, S, warp_stack, Wn);
    if (rc != NMI_OK) return rc;
    DeviceGuard guard(ctx->device);
    const int64_t total = (int64_t)S * Wn;
    rc = ensure_cover_work(ctx, total);
    if (rc != NMI_OK) return rc;

    rc = enqueue_grid_covered(ctx, render_stack, render_masks, S, 0, S, warp_stack, warp_masks, Wn, 0, ctx->d_cover_counts, ctx->d_cover_redo,
                              ctx->d_cover_redo_state, d_ratings, nullptr, /*post=*/true);
    if (rc != NMI_OK) return rc;
    ctx->cover_count_n = total;
    unsigned long long key = 0;
    rc = fetch_key(ctx, &key);
    if (rc != NMI_OK) return rc;
    // the rating table must be complete and visible to every stream when the call returns (as nmi_search_grid)
    if (d_ratings) NMI_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return nmi_key_unpack(key, h_best_index, h_best_score);
}

int nmi_last_cover_counts(nmi_ctx *ctx, int32_t *h_counts, int32_t n)
{
    if (!ctx || !h_counts || n < 0 || n > ctx->cover_count_n) return NMI_ERR_INVALID_ARGUMENT;
    if (n == 0) return NMI_OK;
    DeviceGuard guard(ctx->device);
    NMI_HIP_TRY(ctx, hipMemcpyAsync(h_counts, ctx->d_cover_counts, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    NMI_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return NMI_OK;
}

int nmi_render_points_masked(nmi_ctx *ctx, const float *d_xyz, const float *d_red, int64_t n_points, const float *h_mvps, int32_t S,
                             float point_size, uint8_t *d_render_stack, uint8_t *d_render_masks)
{
    if (!ctx || !d_render_masks) return NMI_ERR_INVALID_ARGUMENT;
    return render_points_impl(ctx, d_xyz, d_red, n_points, h_mvps, S, point_size, d_render_stack, d_render_masks);
}

int nmi_render_mesh_masked(nmi_ctx *ctx, const float *d_xyz, const float *d_uv, int64_t n_triangles, const nmi_texture *tex,
                           const float *h_mvps, int32_t S, uint8_t *d_render_stack, uint8_t *d_render_masks)
{
    if (!ctx || !d_render_masks) return NMI_ERR_INVALID_ARGUMENT;
    return render_mesh_impl(ctx, d_xyz, d_uv, n_triangles, tex, h_mvps, S, d_render_stack, d_render_masks);
}

int nmi_pack_mask_bits(nmi_ctx *ctx, const uint8_t *d_masks, int32_t n, uint8_t *d_bits)
{
    if (!ctx || n < 0 || (n > 0 && (!d_masks || !d_bits))) return NMI_ERR_INVALID_ARGUMENT;
    if (n == 0) return NMI_OK;
    DeviceGuard guard(ctx->device);
    NMI_HIP_TRY(ctx, nmi::launch_pack_mask_bits(d_masks, n, ctx->npix, d_bits, ctx->stream));
    return NMI_OK;
}

}  // extern "C"
