// nmi_masked.h -- internal interface of the masked search (nmi_masked_kernel.hip) and of the warp-mask producer
// (nmi_masked_producer.hip), used by nmi_capi_masked.cpp.  A header of its own so that nothing the existing kernels compile
// (nmi_kernels.h, GridArgs) changes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nmi_kernels.h"

namespace nmi {

// Arguments of nmi_masked_grid_kernel: everything nmi_grid_kernel takes, plus the masks and the per-warp term tables.
// g.table is not read (each candidate uses tables + w * (npix + 1)); g.plan must be null (no content probe).
struct MaskedGridArgs {
    GridArgs g;
    const uint8_t *warp_masks;  // [Wn][H][W], nonzero = the pixel takes part
    const float *tables;        // [Wn][npix + 1]: term[c] for len = counts[w] (entries above counts[w] are not meaningful)
    const int32_t *counts;      // [Wn]: len_w = number of nonzero mask bytes of warp w
    int vec_ok;                 // g.vec_ok and the masks 16-byte aligned: whole aligned 16-byte chunks; else the byte path
    // Candidates whose optimistic pass wrapped a counter, scored again by the exact launch that follows (launch_grid_masked).
    // redo_n and redo_done are zero between searches (the exact launch leaves them so).  Null: exact from the start.
    int32_t *redo;              // [S * Wn]
    uint32_t *redo_n, *redo_done;
};

// counts[w] = nonzero bytes of masks[w] (one workgroup per warp; no atomics, nothing to clear first)
hipError_t launch_mask_counts(const uint8_t *masks, int Wn, int npix, int32_t *counts, hipStream_t stream);
// tables[w][c] = fl32(p * fl32(log2_f64(p))), p = fl32(c / counts[w]), 0 for c = 0 -- nmi_table_kernel's expression per warp.
// Entries above counts[w] are written (as 0) only below the LDS copy's size; a warp with counts[w] = 0 gets zeros.
hipError_t launch_mask_tables(const int32_t *counts, int Wn, int npix, float *tables, hipStream_t stream);
// exact: histogram with returning atomics and wrap bookkeeping from the start (needed for the background rule off with
// fewer than 256 bins, and NMI_OPT_HIST_VARIANT 1); otherwise an optimistic launch and an exact launch for the candidates
// whose count test failed (m.redo must be set).  Either way the last launch posts the winner (m.g.mailbox / out_key).
hipError_t launch_grid_masked(const MaskedGridArgs &m, int workgroups, bool use_bg, bool exact, hipStream_t stream);
// A masked level's count and table nodes (nmi_masked_level.hip).  counts[w] = nonzero bytes of masks[w]; changed[w] = counts[w]
// differs from prev[w], which then takes the new count (prev = -1: every warp changed).  The table launch rebuilds
// launch_mask_tables' entries for the changed warps only.
hipError_t launch_level_mask_counts(const uint8_t *masks, int Wn, int npix, int32_t *counts, int32_t *prev, int32_t *changed, hipStream_t stream);
hipError_t launch_level_mask_tables(const int32_t *counts, const int32_t *changed, int Wn, int npix, float *tables, hipStream_t stream);
// Mid-size grids (nmi_masked_pix_kernel.hip): pix_parts workgroups per candidate over dealt pixel ranges, nmi_pix_kernel's
// hand-off through m.g.blocks (pix_block_bytes, zero when allocated; tag from m.g.epoch + *replay).  Candidates that wrap a
// counter or whose helper does not arrive in time are scored exactly by their owner inside the launch and counted in *healed.
// Needs m.g.order == nullptr, m.g.epoch != 0, width >= 32; m.redo is not used.  Posts the winner like launch_grid_masked.
hipError_t launch_pix_masked(const MaskedGridArgs &m, int pix_parts, double owner_share, bool use_bg, const uint32_t *replay, uint32_t *healed,
                             hipStream_t stream);
// out_masks[w][y][x] = 1 if warp w's pixel (x, y) interpolates from inside the frame (and from nonzero frame_mask taps when
// frame_mask is given), else 0.  coeffs: [Wn][9] inverse maps, as launch_warp.
hipError_t launch_warp_masks(const uint8_t *frame_mask, const float *coeffs, uint8_t *out_masks, int width, int height, int Wn,
                             hipStream_t stream);

}  // namespace nmi
