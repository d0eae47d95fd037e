// nmi_covered.h -- internal interface of the covered search (nmi_covered_kernel.hip: masks on the camera side AND on the map
// side), used by nmi_capi_covered.cpp.  A header of its own so that nothing the existing kernels compile changes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nmi_kernels.h"

namespace nmi {

// Arguments of nmi_covered_grid_kernel: everything nmi_grid_kernel takes, plus the two mask stacks.  g.table is not read
// (each candidate evaluates its own terms from its len); g.plan must be null (no content probe).
struct CoveredGridArgs {
    GridArgs g;
    const uint8_t *warp_masks;    // [Wn][H][W], warp-stack layout; nonzero = the pixel takes part
    const uint8_t *render_masks;  // [S][H][W], render-stack layout (bottom-up rows when g.flip); nonzero = the map covers it
    int32_t *counts;              // [Wn][S] out: len of every candidate scored
    int vec_ok;                   // g.vec_ok and both masks 16-byte aligned: whole aligned 16-byte chunks; else the byte path
    // Candidates whose optimistic pass wrapped a counter, scored again by the exact launch that follows (launch_grid_covered).
    // redo_n and redo_done are zero between searches (the exact launch leaves them so).  Null: exact from the start.
    int32_t *redo;                // [S * Wn]
    uint32_t *redo_n, *redo_done;
};

// exact: histogram with returning atomics and wrap bookkeeping from the start (forced for the background rule off with fewer
// than 256 bins); otherwise an optimistic launch and an exact launch for the candidates whose count test failed (m.redo must
// be set).  Either way the last launch posts the winner (m.g.mailbox / out_key).
hipError_t launch_grid_covered(const CoveredGridArgs &m, int workgroups, bool use_bg, bool exact, hipStream_t stream);
// Mid-size grids (nmi_covered_pix_kernel.hip): pix_parts workgroups per candidate over dealt pixel ranges, nmi_pix_kernel's
// hand-off through m.g.blocks (pix_block_bytes, zero when allocated; tag from m.g.epoch + *replay); len[w][s] is the sum of the
// ranges' counts.  Candidates that wrap a counter or whose helper does not arrive in time are scored exactly by their owner
// inside the launch and counted in *healed.  Needs m.g.order == nullptr, m.g.epoch != 0, width >= 32, and every covered
// pixel added (the background rule on, or off at 256 bins); m.redo is not used.  Writes m.counts and posts the winner like
// launch_grid_covered.
hipError_t launch_pix_covered(const CoveredGridArgs &m, int pix_parts, double owner_share, bool use_bg, const uint32_t *replay, uint32_t *healed,
                              hipStream_t stream);

}  // namespace nmi
