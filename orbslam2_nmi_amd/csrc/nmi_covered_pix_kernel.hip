// nmi_covered_pix_kernel.hip -- the covered search for MID-SIZE grids (33 ... 128 candidates on 256 compute units, and the
// grids plan_search sends here on frames whose rows are not whole aligned chunks): nmi_pix_kernel's pixel ranges (P workgroups
// per candidate, an owner and P - 1 helpers, dealt pieces of the frame) with nmi_covered_grid_kernel's masks on both sides and
// per-candidate len.  nmi_covered_grid_kernel gives a candidate to one workgroup, so 81 candidates fill 81 of the 256 CUs;
// here they fill 243.
//
// The kernel below is a sequence of steps shared with the other two pixel-range kernels (nmi_pix_device.h): pix_unit,
// clear_counters, the masked dealt loop with the chunk mask both_nonzero(warp mask, render mask) (masked_histogram_dealt
// <.., true>), the hand-off (pix_publish / pix_collect, with the range's pixel count in the header) and the owner's merged
// decode with the candidate's own terms (decode_merged with CoverTerms).  Its own: cover_terms below.  From
// nmi_mask_device.h: the term expression (cover_term), the final trees (covered_final_phase) and the heal's exact path
// (covered_histogram_phase, covered_decode_phase).  Results are bit-identical to nmi_covered_grid_kernel's: the decoded
// counters are the same sums, the trees the same code, the terms the same expression of the same len.
//
// What differs from nmi_masked_pix_kernel, and why:
//   * len from the ranges.  Each workgroup counts the pixels of its range whose two mask bytes are both nonzero; a helper hands
//     that count over in its block's header (stored before the drain that precedes its tagged granules, so an owner that sees
//     a tag has it), and the owner sums all ranges.  That sum is len[w][s], and it serves twice: as the expected decoded total
//     of the count test (a wrapped 16-bit field always loses weight, so the decoded sum falls short iff something wrapped) and
//     as the terms' denominator.  The two are the same number only because every covered pixel is added -- the background
//     rule on, or off at 256 bins (row / column 0 cleared in the decode).  The background rule off with fewer than 256 bins
//     drops pixels by their raw values, which would make them differ; plan_search never sends that case to a pixel-range kernel.
//   * Terms.  Known only once every hand-off has arrived: the owner then evaluates the low terms (c <= min(len, kLdsTable - 1))
//     into lds.table with cover_term, and counts at or above kLdsTable are evaluated inline during the merged decode and the
//     final trees, as covered_decode_phase does.  No global table is read.
//   * Outputs.  The owner writes counts[w][s] (nmi_last_cover_counts), the rating, and posts the winner like
//     launch_grid_covered.
//   * Heal.  A candidate that fails the count test, or whose helper did not arrive within the bounded wait, is scored by its
//     owner alone on the covered exact path (covered_histogram_phase with returning atomics + wrap bookkeeping,
//     covered_decode_phase, covered_final_phase) inside the launch; both are counted in healed[kPixHealed] (nmi_pix_status().healed) and each under its
//     cause (nmi_pix_heal_counts).
//   * Shapes.  Rows need not be whole aligned chunks: the dealt chunks take nmi_pix_kernel's unaligned-row addressing for the
//     frame, the render and both masks alike (the render mask in the render's row order), and the owner adds the rows' last
//     width % 16 pixels one by one (frames of at least 32 pixels of width, e.g. 1241 x 376).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nmi_mask_device.h"  // cover_term, covered_final_phase; covered_histogram_phase, covered_decode_phase (the exact path)
#include "nmi_pix_device.h"   // pix_unit, clear_counters, masked_histogram_dealt, pix_publish / pix_collect, decode_merged, CoverTerms

namespace nmi {

namespace {

// lds.table[c] = cover_term(c, len) for c <= min(len, kLdsTable - 1); entries above len are never read (every count is <= len
// unless a field wrapped, and then the count test rejects the candidate)
__device__ __forceinline__ void cover_terms(Lds &lds, uint32_t len, int tid)
{
    const uint32_t top = min(len, (uint32_t)kLdsTable - 1u);
#pragma unroll
    for (int k = 0; k < kLdsTable / kBlock; ++k) {
        const uint32_t c = (uint32_t)(tid + k * kBlock);
        if (c <= top) lds.table[c] = cover_term(c, len);
    }
}

}  // namespace

// ZERO0: background rule off at 256 bins (row / column 0 cleared in the decode).
template <bool ZERO0, bool SHIFTED>
__global__ __launch_bounds__(NMI_BLOCK_THREADS) void nmi_covered_pix_kernel(CoveredGridArgs m, int P, DealArgs dealing, const uint32_t *replay,
                                                                           uint32_t *healed)
{
    __shared__ Lds lds;
    const GridArgs &a = m.g;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;

    const PixUnit u = pix_unit(a, P, dealing, replay);
    const int p = u.p, w = u.w, s = u.s;
    const uint8_t *render = a.render_stack + (size_t)s * a.npix;
    const uint8_t *warped = a.warp_stack + (size_t)w * a.npix;
    const uint8_t *wmask = m.warp_masks + (size_t)w * a.npix;
    const uint8_t *rmask = m.render_masks + (size_t)s * a.npix;

    if (blockIdx.x == 0 && tid == 0 && a.reset_key) *a.reset_key = 0ull;  // next launch's slot; idle during this one
    clear_counters(lds, tid);
    const Deal deal = make_deal(dealing, P, u.q);
    __syncthreads();
    add_count(&lds.total[1], masked_histogram_dealt<SHIFTED, true>(lds, a, render, warped, wmask, rmask, wave, lane, deal), lane);

    if (u.q != 0) {
        __syncthreads();
        pix_publish<false>(lds, a, u, wave, lane);
        return;
    }

    // ---- owner ----
    u32x4 acc[kUnitsPerLane];
    pix_collect<false>(lds, u, P, wave, lane, acc);
    __syncthreads();  // B1: every wavefront's pixels are in the counters, every helper's count in total[1] (= len)
    unsigned long long prev_key = 0;
    bool alone = lds.fallback != 0;  // some wave gave up on a helper (workgroup-uniform)
    if (!alone) {
        const uint32_t len = lds.total[1];
        cover_terms(lds, len, tid);
        __syncthreads();  // B1b: the candidate's low terms are in lds.table
        decode_merged<ZERO0>(lds, CoverTerms{len}, wave, lane, acc);
        __syncthreads();
        alone = lds.total[0] != len;  // some 16-bit field wrapped (workgroup-uniform, rare)
        if (!alone && wave == 0) {
            if (lane == 0) m.counts[p] = (int32_t)len;
            covered_final_phase(lds, a, len, lane, p, w, s, prev_key);
        }
    }
    if (alone) {
        // cold: this candidate once more, by this workgroup alone, on the covered exact path
        if (tid == 0 && healed) pix_count_heal(healed, lds.fallback != 0, true);
        __syncthreads();
        clear_counters(lds, tid);
        __syncthreads();
        const uint32_t n = covered_histogram_phase<true, SHIFTED, 1>(lds, 0, m, render, warped, wmask, rmask, tid);
        add_count(&lds.total[1], n, lane);
        __syncthreads();
        const uint32_t len = lds.total[1];
        cover_terms(lds, len, tid);
        __syncthreads();
        covered_decode_phase<ZERO0>(lds, 0, len, wave, lane);
        __syncthreads();
        if (wave == 0) {
            if (lane == 0) m.counts[p] = (int32_t)len;
            covered_final_phase(lds, a, len, lane, p, w, s, prev_key);
        }
    }
    if (wave == 0) finish_search(a, lane, prev_key, (uint32_t)u.total);
}

// One launch of total * pix_parts workgroups (nmi_covered.h).
hipError_t launch_pix_covered(const CoveredGridArgs &m, int pix_parts, double owner_share, bool use_bg, const uint32_t *replay, uint32_t *healed,
                              hipStream_t stream)
{
    const GridArgs &a = m.g;
    if (!pix_launch_ok(a, pix_parts, use_bg) || a.plan || !m.counts || !m.warp_masks || !m.render_masks) return hipErrorInvalidValue;
    return pix_launch(a, pix_parts, owner_share, use_bg, [&](auto zero0, auto shifted, dim3 grid, const DealArgs &g) {
        hipLaunchKernelGGL((nmi_covered_pix_kernel<decltype(zero0)::value, decltype(shifted)::value>), grid, dim3(kBlock), 0, stream, m, pix_parts, g, replay, healed);
    });
}

}  // namespace nmi
