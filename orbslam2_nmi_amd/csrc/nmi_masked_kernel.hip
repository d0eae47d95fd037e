// nmi_masked_kernel.hip -- the masked grid search: nmi_grid_kernel's computation with a per-warp pixel mask.
//
// A candidate (warp w, render s) counts pixel pos iff mask[w][pos] != 0 and the background rule passes (NMI.cu:85, on the
// raw intensities, before the shift); the entropy terms use len_w = popcount(mask[w]) in place of W*H (NMI.cu:245), so each
// warp has its own per-count table.  Everything else -- the trees, SUC / ENMI, the all-zero guard, the rating table and the
// arg-max -- is nmi_grid_kernel's own code (nmi_grid_device.h; the masked forms are in nmi_mask_device.h).
//
// What changes against nmi_grid_kernel, and why:
//   * Pixel loop.  A wavefront whose 16-byte mask chunks are all nonzero runs nmi_grid_kernel's add_chunk unchanged; one with
//     a partly masked chunk adds pixel by pixel with excluded lanes issuing no LDS atomic.  The kernel is bound by the LDS atomic rate
//     (DESIGN.md section 4), so the extra 16-byte mask load per chunk -- the same mask for all S renders of a warp, hence an
//     L2 hit under the XCD tiling order -- and the few VALU of the test ride in the shadow of the atomics.
//   * Wrap detector.  The optimistic pass compares the sum of the decoded counters with the pixels it actually added:
//     len_w (background rule on; off at 256 bins, where every masked pixel is counted and row / column 0 are cleared after).
//   * Flat chunks are not folded (fold_flat_chunk's side counters assume every pixel of a chunk counts): a flat region only
//     costs time, and a bin above 65535 fails the count test and is redone on the exact path like any other wrap.
//   * Exact redo.  nmi_grid_kernel redoes wrapped candidates in a cold loop of the same kernel; here that loop took the
//     kernel past its 128 VGPRs into scratch, so failing candidates go to a list that a second, exact launch scores (it
//     returns at once when the list is empty).
//   * Term tables.  Each candidate decodes with its warp's table.  The LDS copy of the low entries (kLdsTable floats) is
//     reloaded whenever a workgroup's next candidate has another warp -- under the XCD tiling order almost every candidate:
//     4 loads + 4 LDS stores per lane (loads issued before the histogram phase, stored after it where registers allow, as
//     nmi_grid_kernel does for its first candidate), against npix / 1024 atomics per lane (300 at 640 x 480).  Visiting the
//     candidates warp by warp instead would give up the tiling that keeps an XCD's images in its L2.
//   * Shapes.  Whole aligned 16-byte chunks (width % 16 == 0, width >= 32, stacks and masks 16-byte aligned) take the
//     16-byte path; every other shape takes a byte path (correct, slower per pixel).  No split, pixel-range or few-levels form.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nmi_mask_device.h"

namespace nmi {

// One workgroup per candidate, grid-stride over the candidates in the visiting order -- nmi_grid_kernel's structure: B1
// histogram -> decode, B2 decode -> (wavefront 0: final trees + score + arg-max) || (the others: next candidate's pixels),
// per-candidate state double-buffered by parity.
//   HIST 3: optimistic pass (non-returning atomics) and the count test.  A candidate that fails it is not scored: it is
//           appended to m.redo, and the HIST 1 launch that follows (m.redo set there too) scores it exactly ("Exact redo" above).
//   HIST 1: exact throughout -- every candidate of the grid (m.redo null), or the candidates m.redo lists.
template <bool BG, bool SHIFTED, int HIST>
__global__ __launch_bounds__(NMI_BLOCK_THREADS) void nmi_masked_grid_kernel(MaskedGridArgs m)
{
    __shared__ Lds lds;
    const GridArgs &a = m.g;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    constexpr bool kOptimistic = HIST == 3;
    constexpr int kFirst = kOptimistic ? 2 : HIST;
    // Background rule off at 256 bins: count every masked pixel (the detector's expected total is then len_w) and clear row /
    // column 0 in decode_phase, as nmi_grid_kernel does with W*H -- on the optimistic pass and on its redo alike.
    constexpr bool kZero0 = !BG && !SHIFTED && (kOptimistic || HIST == 1);
    constexpr bool kCountAll = BG || kZero0;
    constexpr bool kParkTable = kOptimistic && !kZero0;
    const bool from_list = !kOptimistic && m.redo != nullptr;
    const int total = from_list ? (int)__hip_atomic_load(m.redo_n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : a.S_local * a.Wn;

    if (blockIdx.x == 0 && tid == 0 && a.reset_key) *a.reset_key = 0ull;  // next launch's slot; idle during this one
    unsigned long long prev_key = 0;
    const int slot = from_list ? (int)blockIdx.x : slot_in_round(blockIdx.x, gridDim.x);
    if (slot < total) {
        clear_lds(lds, tid);
        __syncthreads();
    }
    const size_t stride = (size_t)a.npix + 1;
    int par = 0;
    int table_w = -1;  // warp whose low table entries are in LDS (workgroup-uniform)
    for (int ordinal = slot; ordinal < total; ordinal += gridDim.x, par ^= 1) {
        const int p = from_list ? m.redo[ordinal] : candidate_at(a, ordinal);
        const int w = p / a.S_local;
        const int s = p - w * a.S_local;
        GridArgs aw = a;
        aw.table = m.tables + (size_t)w * stride;
        // The LDS copy of the warp's low table entries.  Every wavefront is past the previous candidate's decode (B2), the only
        // reader of lds.table.  The optimistic pass parks the loads in registers across its histogram phase (their latency
        // hidden); the exact pass and the background-rule-off pass -- at their register cap -- store them at once.
        const bool reload = w != table_w;
        float tab[kLdsTable / kBlock];
        if (reload) {
#pragma unroll
            for (int k = 0; k < kLdsTable / kBlock; ++k) {
                const int c = tid + k * kBlock;
                tab[k] = aw.table[c <= a.npix ? c : 0];
                if (!kParkTable) lds.table[c] = tab[k];
            }
        }
        masked_histogram_phase<kCountAll, SHIFTED, kFirst>(lds, par, m, a.render_stack + (size_t)s * a.npix, a.warp_stack + (size_t)w * a.npix,
                                                           m.warp_masks + (size_t)w * a.npix, tid);
        if (reload) {
            if (kParkTable) {
#pragma unroll
                for (int k = 0; k < kLdsTable / kBlock; ++k) lds.table[tid + k * kBlock] = tab[k];
            }
            table_w = w;
        }
        __syncthreads();  // B1
        decode_phase<kZero0>(lds, par, aw, wave, lane);
        __syncthreads();  // B2
        if (wave == 0) {
            // a 16-bit counter wrapped (the sum of the decoded counters falls short of the pixels added): leave it to the redo
            if (kOptimistic && lds.total[par] != (uint32_t)m.counts[w]) {
                if (lane == 0) redo_append(m, p);
            } else {
                final_phase(lds, aw, lane, p, w, s, prev_key);
            }
            retire_candidate(lds, par, lane);
        }
    }

    if (wave == 0) {
        if (from_list && lane == 0) redo_consumed(m);
        finish_search(a, lane, prev_key, gridDim.x);
    }
}

// One workgroup per warp.
__global__ __launch_bounds__(1024) void nmi_mask_count_kernel(const uint8_t *__restrict__ masks, int npix, int32_t *__restrict__ counts)
{
    __shared__ uint32_t part[16];
    const int w = blockIdx.x, tid = threadIdx.x;
    const uint8_t *m = masks + (size_t)w * npix;
    const int head = min((int)((16u - ((uintptr_t)m & 15u)) & 15u), npix);  // bytes before the first aligned 16-byte unit
    const int units = (npix - head) >> 4;
    uint32_t n = 0;
    for (int i = tid; i < head; i += 1024) n += m[i] != 0;
    const uint4 *u = reinterpret_cast<const uint4 *>(m + head);
    for (int i = tid; i < units; i += 1024) {
        const uint4 v = u[i];
        n += __popc(nonzero_byte_bits(v.x)) + __popc(nonzero_byte_bits(v.y)) + __popc(nonzero_byte_bits(v.z)) + __popc(nonzero_byte_bits(v.w));
    }
    for (int i = head + units * 16 + tid; i < npix; i += 1024) n += m[i] != 0;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) n += (uint32_t)__shfl_xor((int)n, off, 64);
    if ((tid & 63) == 0) part[tid >> 6] = n;
    __syncthreads();
    if (tid == 0) {
        uint32_t t = 0;
        for (int k = 0; k < 16; ++k) t += part[k];
        counts[w] = (int32_t)t;
    }
}

// nmi_table_kernel's expression with len = counts[w].
__global__ __launch_bounds__(256) void nmi_mask_table_kernel(const int32_t *__restrict__ counts, int npix, float *__restrict__ tables)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    const int w = blockIdx.y;
    if (c > npix) return;
    const int len = counts[w];
    float v = 0.0f;
    if (c > len) {
        if (c >= kLdsTable) return;  // never read: joint and marginal counts are <= len; only the LDS copy reads up to kLdsTable - 1
    } else if (c > 0) {
        const float p = (float)c / (float)len;
        const float l = (float)log2((double)p);
        v = p * l;
    }
    tables[(size_t)w * ((size_t)npix + 1) + c] = v;
}

hipError_t launch_mask_counts(const uint8_t *masks, int Wn, int npix, int32_t *counts, hipStream_t stream)
{
    hipLaunchKernelGGL(nmi_mask_count_kernel, dim3(Wn), dim3(1024), 0, stream, masks, npix, counts);
    return hipGetLastError();
}

hipError_t launch_mask_tables(const int32_t *counts, int Wn, int npix, float *tables, hipStream_t stream)
{
    const int threads = 256;
    hipLaunchKernelGGL(nmi_mask_table_kernel, dim3((npix + 1 + threads - 1) / threads, Wn), dim3(threads), 0, stream, counts, npix, tables);
    return hipGetLastError();
}

hipError_t launch_grid_masked(const MaskedGridArgs &m, int workgroups, bool use_bg, bool exact, hipStream_t stream)
{
    const bool shifted = m.g.shift != 0;
    exact = exact || (!use_bg && shifted);  // BG off below 256 bins: the rule looks at raw values, bin 0 also holds 1 .. 2^shift - 1
    if (m.g.plan || (!exact && (!m.redo || !m.redo_n || !m.redo_done))) return hipErrorInvalidValue;
    with_bg_shifted(use_bg, shifted, [&](auto bg, auto sh) {
        launch_redo_pair<MaskedGridArgs>(nmi_masked_grid_kernel<bg.value, sh.value, 3>, nmi_masked_grid_kernel<bg.value, sh.value, 1>, m, workgroups, exact, stream);
    });
    return hipGetLastError();
}

}  // namespace nmi
