// nmi_masked_pix_kernel.hip -- the masked search for MID-SIZE grids (33 ... 128 candidates on 256 compute units): nmi_pix_kernel's
// pixel ranges (P workgroups per candidate, an owner and P - 1 helpers, dealt pieces of the frame) with nmi_masked_grid_kernel's
// per-warp masks and term tables.  nmi_masked_grid_kernel gives a candidate to one workgroup, so 81 candidates fill 81 of
// the 256 CUs; here they fill 243.
//
// The kernel below is a sequence of steps shared with the other two pixel-range kernels (nmi_pix_device.h): pix_unit,
// clear_counters, the masked dealt loop (masked_histogram_dealt, which the covered kernel uses with both masks; it adds with
// masked_add_chunk of nmi_mask_device.h: whole-chunk test, then add_chunk unchanged, per-pixel predication only on mixed
// chunks), the hand-off (pix_publish / pix_collect, with the range's pixel count in the header where nmi_pix_kernel sends side
// counters), the owner's merged decode (decode_merged with TableTerms) and final trees (final_phase_owner); the heal runs the
// exact path of nmi_mask_device.h (masked_histogram_phase).  Results are bit-identical to nmi_masked_grid_kernel's: the
// decoded counters are the same sums, the trees the same code, the terms the same table.
//
// What differs from nmi_pix_kernel, and why:
//   * Count test.  The expected total is no longer W*H: each workgroup counts the pixels it added (the nonzero mask bytes of
//     its chunks; with the background rule on, or off at 256 bins, every masked pixel is added), a helper hands that count over
//     in its block's header (stored before the drain that precedes its tagged granules, so an owner that sees a tag has it), and
//     the owner compares its decoded total with the sum over all ranges.  A wrapped 16-bit field always loses weight, in a
//     helper, in the owner or in the merge, so the sum falls short iff something wrapped.
//   * Flat chunks are not folded (as in nmi_masked_grid_kernel: fold_flat_chunk's side counters assume every pixel of a chunk
//     counts); helpers' side counters are therefore always empty and are not handed over.
//   * Heal.  A candidate that fails the count test, or whose helper did not arrive within the bounded wait, is scored by its
//     owner alone on the masked exact path (masked_histogram_phase with returning atomics + wrap bookkeeping, decode_phase,
//     final_phase) inside the launch; both are counted in healed[kPixHealed] (nmi_pix_status().healed) and each under its
//     cause (nmi_pix_heal_counts).
//   * Tables.  The owner decodes with tables + w * (npix + 1) (its LDS copy of the low entries loaded once: one candidate per
//     workgroup).
//   * Shapes.  Rows need not be whole aligned chunks: the dealt chunks take nmi_pix_kernel's unaligned-row addressing for the
//     frame, the render and the mask alike, and the owner adds the rows' last width % 16 pixels one by one (frames of at least
//     32 pixels of width, e.g. 1241 x 376).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nmi_mask_device.h"  // masked_histogram_phase (the exact path)
#include "nmi_pix_device.h"   // pix_unit, clear_counters, masked_histogram_dealt, pix_publish / pix_collect, decode_merged, final_phase_owner

namespace nmi {

// ZERO0: background rule off at 256 bins (row / column 0 cleared in the decode).
template <bool ZERO0, bool SHIFTED>
__global__ __launch_bounds__(NMI_BLOCK_THREADS) void nmi_masked_pix_kernel(MaskedGridArgs m, int P, DealArgs dealing, const uint32_t *replay,
                                                                          uint32_t *healed)
{
    __shared__ Lds lds;
    const GridArgs &a = m.g;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;

    const PixUnit u = pix_unit(a, P, dealing, replay);
    const int p = u.p, w = u.w, s = u.s;
    const bool owner = u.q == 0;
    const uint8_t *render = a.render_stack + (size_t)s * a.npix;
    const uint8_t *warped = a.warp_stack + (size_t)w * a.npix;
    const uint8_t *mask = m.warp_masks + (size_t)w * a.npix;

    if (blockIdx.x == 0 && tid == 0 && a.reset_key) *a.reset_key = 0ull;  // next launch's slot; idle during this one
    GridArgs aw = a;
    aw.table = m.tables + (size_t)w * ((size_t)a.npix + 1);
    float tab[kLdsTable / kBlock];
    if (owner) {
#pragma unroll
        for (int k = 0; k < kLdsTable / kBlock; ++k) {
            const int c = tid + k * kBlock;
            tab[k] = aw.table[c <= a.npix ? c : 0];
        }
    }
    clear_counters(lds, tid);
    const Deal deal = make_deal(dealing, P, u.q);
    __syncthreads();
    add_count(&lds.total[1], masked_histogram_dealt<SHIFTED, false>(lds, a, render, warped, mask, nullptr, wave, lane, deal), lane);

    if (!owner) {
        __syncthreads();
        pix_publish<false>(lds, a, u, wave, lane);
        return;
    }

    // ---- owner ----
#pragma unroll
    for (int k = 0; k < kLdsTable / kBlock; ++k) lds.table[tid + k * kBlock] = tab[k];
    u32x4 acc[kUnitsPerLane];
    pix_collect<false>(lds, u, P, wave, lane, acc);
    __syncthreads();  // B1: every wavefront's pixels are in the counters, every helper's count in total[1]
    unsigned long long prev_key = 0;
    bool alone = lds.fallback != 0;  // some wave gave up on a helper (workgroup-uniform)
    if (!alone) {
        decode_merged<ZERO0>(lds, TableTerms{aw.table, (uint32_t)a.npix, a.dbg_joint}, wave, lane, acc);
        __syncthreads();
        alone = lds.total[0] != lds.total[1];  // some 16-bit field wrapped (workgroup-uniform, rare)
        if (!alone && wave == 0) final_phase_owner(lds, aw, lane, p, w, s, prev_key);
    }
    if (alone) {
        // cold: this candidate once more, by this workgroup alone, on the masked exact path
        if (tid == 0 && healed) pix_count_heal(healed, lds.fallback != 0, true);
        __syncthreads();
        clear_counters(lds, tid);
        __syncthreads();
        masked_histogram_phase<true, SHIFTED, 1>(lds, 0, m, render, warped, mask, tid);
        __syncthreads();
        decode_phase<ZERO0>(lds, 0, aw, wave, lane);
        __syncthreads();
        if (wave == 0) final_phase(lds, aw, lane, p, w, s, prev_key);
    }
    if (wave == 0) finish_search(a, lane, prev_key, (uint32_t)u.total);
}

// One launch of total * pix_parts workgroups (nmi_masked.h).
hipError_t launch_pix_masked(const MaskedGridArgs &m, int pix_parts, double owner_share, bool use_bg, const uint32_t *replay, uint32_t *healed,
                             hipStream_t stream)
{
    const GridArgs &a = m.g;
    if (!pix_launch_ok(a, pix_parts, use_bg) || a.plan || !m.tables || !m.warp_masks) return hipErrorInvalidValue;
    return pix_launch(a, pix_parts, owner_share, use_bg, [&](auto zero0, auto shifted, dim3 grid, const DealArgs &g) {
        hipLaunchKernelGGL((nmi_masked_pix_kernel<decltype(zero0)::value, decltype(shifted)::value>), grid, dim3(kBlock), 0, stream, m, pix_parts, g, replay, healed);
    });
}

}  // namespace nmi
