// nmi_covered_kernel.hip -- the covered search: nmi_masked_grid_kernel's computation with a mask on BOTH sides, a per-warp
// mask of the camera frame and a per-render coverage mask of the map.
//
// A candidate (warp w, render s) counts pixel pos iff warp_masks[w][pos] != 0, render_masks[s][rpos] != 0 (rpos: the render
// pixel nmi_search_grid pairs with pos, row-flipped when render_bottom_up) and the background rule passes on the raw
// intensities (NMI.cu:85).  len[w][s] = the number of pos where both masks are nonzero (not reduced by the background rule,
// like W*H) replaces W*H in the term fl32(p * fl32(log2_f64(p))), p = fl32(c / len) -- nmi_mask_table_kernel's expression.
// Everything else -- the trees, SUC / ENMI, the all-zero guard, the rating table and the arg-max -- is nmi_grid_kernel's own
// code (nmi_grid_device.h), the pixel forms are nmi_masked_grid_kernel's (nmi_mask_device.h).
//
// What changes against nmi_masked_grid_kernel, and why:
//   * len is per candidate, so there are no global term tables (one per candidate would be 729 x 1.2 MB at 640 x 480).  Each
//     lane counts the pixels it adds whose two mask bytes are both nonzero; after the histogram phase the counts meet in LDS,
//     every lane evaluates its share of the low terms (c <= min(len, kLdsTable - 1)) into lds.table, and the rare counts at or
//     above kLdsTable are evaluated inline, in the decode (covered_decode_phase) and in the final trees.  The cost is one
//     more barrier per candidate and 4 fp64 logarithms per lane.
//   * Pixel loop.  The two mask chunks are folded into one (bit 7 of each byte: both nonzero) and handed to masked_add_chunk
//     unchanged, so a wavefront whose 16 pixels all take part runs add_chunk, the unmasked hot form.  Masks mean "nonzero":
//     the bytes are tested, never ANDed raw (0x01 & 0x02 == 0).
//   * Wrap detector and redo: nmi_masked_grid_kernel's rules with the expected total taken from the in-kernel len.
//   * Shapes.  Whole aligned 16-byte chunks (width % 16 == 0, width >= 32, both stacks and both masks 16-byte aligned) take the
//     16-byte path; every other shape takes a byte path.  No split or few-levels form; mid-size grids
//     take the pixel-range form of nmi_covered_pix_kernel.hip.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nmi_mask_device.h"

namespace nmi {

// One workgroup per candidate, grid-stride over the candidates in the visiting order -- nmi_masked_grid_kernel's structure
// with one more barrier: B1 histogram -> terms, B1b terms -> decode, B2 decode -> (wavefront 0: final trees + score + arg-max)
// || (the others: next candidate's pixels).  lds.table holds the candidate's terms from B1b until wavefront 0 has finished
// its final trees, which is before anyone passes the next B1.
//   HIST 3: optimistic pass (non-returning atomics) and the count test against len; a candidate that fails it goes to m.redo.
//   HIST 1: exact throughout -- every candidate of the grid (m.redo null), or the candidates m.redo lists.
template <bool BG, bool SHIFTED, int HIST>
__global__ __launch_bounds__(NMI_BLOCK_THREADS) void nmi_covered_grid_kernel(CoveredGridArgs m)
{
    __shared__ Lds lds;
    __shared__ uint32_t cover_part[kBlock / 64];  // per wavefront: pixels taking part
    const GridArgs &a = m.g;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    constexpr bool kOptimistic = HIST == 3;
    constexpr int kFirst = kOptimistic ? 2 : HIST;
    // Background rule off at 256 bins: count every covered pixel (the detector's expected total is then len) and clear row /
    // column 0 in the decode, as nmi_masked_grid_kernel does.
    constexpr bool kZero0 = !BG && !SHIFTED && (kOptimistic || HIST == 1);
    constexpr bool kCountAll = BG || kZero0;
    const bool from_list = !kOptimistic && m.redo != nullptr;
    const int total = from_list ? (int)__hip_atomic_load(m.redo_n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : a.S_local * a.Wn;

    if (blockIdx.x == 0 && tid == 0 && a.reset_key) *a.reset_key = 0ull;  // next launch's slot; idle during this one
    unsigned long long prev_key = 0;
    const int slot = from_list ? (int)blockIdx.x : slot_in_round(blockIdx.x, gridDim.x);
    if (slot < total) {
        clear_lds(lds, tid);
        __syncthreads();
    }
    int par = 0;
    for (int ordinal = slot; ordinal < total; ordinal += gridDim.x, par ^= 1) {
        const int p = from_list ? m.redo[ordinal] : candidate_at(a, ordinal);
        const int w = p / a.S_local;
        const int s = p - w * a.S_local;
        uint32_t n = covered_histogram_phase<kCountAll, SHIFTED, kFirst>(lds, par, m, a.render_stack + (size_t)s * a.npix,
                                                                         a.warp_stack + (size_t)w * a.npix, m.warp_masks + (size_t)w * a.npix,
                                                                         m.render_masks + (size_t)s * a.npix, tid);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) n += (uint32_t)__shfl_xor((int)n, off, 64);
        if (lane == 0) cover_part[wave] = n;
        __syncthreads();  // B1
        uint32_t len = 0;
#pragma unroll
        for (int k = 0; k < kBlock / 64; ++k) len += cover_part[k];
        // the candidate's low terms; entries above len are never read (every count is <= len)
        const uint32_t top = min(len, (uint32_t)kLdsTable - 1u);
#pragma unroll
        for (int k = 0; k < kLdsTable / kBlock; ++k) {
            const uint32_t c = (uint32_t)(tid + k * kBlock);
            if (c <= top) lds.table[c] = cover_term(c, len);
        }
        __syncthreads();  // B1b
        covered_decode_phase<kZero0>(lds, par, len, wave, lane);
        __syncthreads();  // B2
        if (wave == 0) {
            if (lane == 0) m.counts[p] = (int32_t)len;
            // a 16-bit counter wrapped (the sum of the decoded counters falls short of the pixels added): leave it to the redo
            if (kOptimistic && lds.total[par] != len) {
                if (lane == 0) redo_append(m, p);
            } else {
                covered_final_phase(lds, a, len, lane, p, w, s, prev_key);
            }
            retire_candidate(lds, par, lane);
        }
    }

    if (wave == 0) {
        if (from_list && lane == 0) redo_consumed(m);
        finish_search(a, lane, prev_key, gridDim.x);
    }
}

hipError_t launch_grid_covered(const CoveredGridArgs &m, int workgroups, bool use_bg, bool exact, hipStream_t stream)
{
    const bool shifted = m.g.shift != 0;
    exact = exact || (!use_bg && shifted);  // BG off below 256 bins: the rule looks at raw values, bin 0 also holds 1 .. 2^shift - 1
    if (m.g.plan || !m.counts || (!exact && (!m.redo || !m.redo_n || !m.redo_done))) return hipErrorInvalidValue;
    with_bg_shifted(use_bg, shifted, [&](auto bg, auto sh) {
        launch_redo_pair<CoveredGridArgs>(nmi_covered_grid_kernel<bg.value, sh.value, 3>, nmi_covered_grid_kernel<bg.value, sh.value, 1>, m, workgroups, exact, stream);
    });
    return hipGetLastError();
}

}  // namespace nmi
