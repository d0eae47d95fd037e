// nmi_capi_covered.cpp -- the covered entry points of include/nmi_hip.h: nmi_search_grid_covered, nmi_last_cover_counts,
// nmi_render_points_masked, nmi_render_mesh_masked.  Kernels: nmi_covered_kernel.hip and nmi_covered_pix_kernel.hip (mid-size
// grids) for the search, nmi_producers.hip and nmi_mesh.hip (the coverage forms of the renderers' last pass); and
// nmi_pack_mask_bits (nmi_mask_bits.hip), which packs such coverage into the bits a covered stream ticket carries.
#include "nmi_ctx.h"
#include "nmi_mask_bits.h"

using namespace nmi_internal;

namespace {

// Counts [total].  Growing waits for the stream (the old buffer may be in use by a search in flight).
int ensure_cover_work(nmi_ctx *ctx, int64_t total)
{
    const size_t bytes = (size_t)total * sizeof(int32_t);
    if (bytes > ctx->d_cover_counts.size()) ctx->cover_count_n = 0;
    NMI_HIP_TRY(ctx, ctx->d_cover_counts.grow(bytes, ctx->stream));
    return NMI_OK;
}

}  // namespace

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
    if (rc == NMI_OK) rc = ensure_mask_redo(ctx, total);
    if (rc != NMI_OK) return rc;

    SearchRequest rq = SearchRequest::block(render_stack, S, 0, S, warp_stack, Wn);
    rq.d_ratings = d_ratings;
    rq.post = true;
    rc = enqueue_grid_mask(ctx, rq, MaskSide{warp_masks, render_masks, ctx->d_cover_counts.as<int32_t>(), nullptr, ctx->d_mask_redo.as<int32_t>(),
                                                ctx->d_mask_redo_state.as<uint32_t>()});
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
    NMI_HIP_TRY(ctx, hipMemcpyAsync(h_counts, ctx->d_cover_counts.as<>(), (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
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
    return render_mesh_impl(ctx, MapKind::textured_mesh, d_xyz, d_uv, n_triangles, tex, h_mvps, S, d_render_stack, d_render_masks);
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
