// nmi_covered_kernel.hip -- the covered search: nmi_masked_grid_kernel's computation with a mask on BOTH sides, a per-warp
// mask of the camera frame and a per-render coverage mask of the map.
//
// A candidate (warp w, render s) counts pixel pos iff warp_masks[w][pos] != 0, render_masks[s][rpos] != 0 (rpos: the render
// pixel nmi_search_grid pairs with pos, row-flipped when render_bottom_up) and the background rule passes on the raw
// intensities (NMI.cu:85).  len[w][s] = the number of pos where both masks are nonzero (not reduced by the background rule,
// like W*H) replaces W*H in the term fl32(p * fl32(log2_f64(p))), p = fl32(c / len) -- nmi_mask_table_kernel's expression.
// Everything else -- the trees, SUC / ENMI, the all-zero guard, the rating table and the arg-max -- is nmi_grid_kernel's own
// code (nmi_kernels.hip, included for its device functions only), the pixel forms are nmi_masked_kernel.hip's.
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

// nmi_covered_pix_kernel.hip includes this file for its device functions only (NMI_COVERED_DEVICE_ONLY), after nmi_kernels.hip
// and nmi_masked_kernel.hip.
#ifndef NMI_COVERED_DEVICE_ONLY
#define NMI_KERNELS_DEVICE_ONLY 1
#include "nmi_kernels.hip"  // Lds, add_chunk, apply_wraps, the trees, commit_score, finish_search, candidate_at
#define NMI_MASKED_DEVICE_ONLY 1
#include "nmi_masked_kernel.hip"  // masked_add_chunk, nonzero_byte_bits
#endif
#include "nmi_covered.h"

namespace nmi {

namespace {

// term of count c for len pixels: nmi_table_kernel's / nmi_mask_table_kernel's expression, bit for bit
__device__ __forceinline__ float cover_term(uint32_t c, uint32_t len)
{
    if (c == 0u) return 0.0f;
    const float p = (float)c / (float)len;
    const float l = (float)log2((double)p);
    return p * l;
}

// ---- decode phase: decode_phase (nmi_kernels.hip) with the candidate's terms -------------------------------------------------
// The same counters, wrap replay, trees and ZERO0 rule, word for word; what differs: counts at or above kLdsTable are
// evaluated (cover_term) instead of read from a global table, and the side counters of fold_flat_chunk and the debug copy are
// left out (neither exists here: the masked pixel forms never fold, and no covered entry point asks for the joint histogram).
// A copy rather than a hook in decode_phase: a hook, even one inlined to the same expression, changed the register allocation
// of nmi_grid_kernel; and the rare branch's fp64 logarithm needs the registers the two left-out parts would hold (with them
// the kernel spilled more; it is at its 128-VGPR cap either way, profiles/covered/README.md).
template <bool ZERO0>
__device__ __forceinline__ void covered_decode_phase(Lds &lds, int par, uint32_t len, int wave, int lane)
{
    const uint32_t novf = lds.ovf_n[par] < (uint32_t)kOvfCap ? lds.ovf_n[par] : (uint32_t)kOvfCap;
    uint32_t wave_total = 0;
    const int i = lane & 15, r = lane >> 4, o = r & 1;
    uint32_t col_lo[8], col_hi[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) col_lo[k] = col_hi[k] = 0;
#pragma unroll 1
    for (int pass = 0; pass < kRowsPerWave / 4; ++pass) {
        const int d1 = wave * kRowsPerWave + pass * 4 + r;
        const uint32_t a0 = d1 * 128 + i + 16 * o;
        uint32_t lo[8], hi[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const uint32_t idx = k < 7 ? a0 + 16 * k : a0 + 112 - 128 * o;
            const uint32_t wd = lds.joint[idx];
            lds.joint[idx] = 0;  // ready for the next candidate
            lo[k] = wd & 0xFFFFu;
            hi[k] = wd >> 16;
        }
        if (__builtin_expect(novf != 0, 0)) {
#pragma unroll
            for (int k = 0; k < 8; ++k) apply_wraps(lds, par, novf, k < 7 ? a0 + 16 * k : a0 + 112 - 128 * o, lo[k], hi[k]);
        }
        uint32_t rsum = 0, cmax = 0;
        if (ZERO0) {
            uint32_t raw = 0;
#pragma unroll
            for (int k = 0; k < 8; ++k) raw += lo[k] + hi[k];
            wave_total += row_sum_16(raw);
            if (i == 0) lo[o ? 7 : 0] = 0;  // the bin d2 = 0 of this row
            if (d1 == 0) {
#pragma unroll
                for (int k = 0; k < 8; ++k) lo[k] = hi[k] = 0;
            }
        }
        float tl[8], th[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            col_lo[k] += lo[k];
            col_hi[k] += hi[k];
            rsum += lo[k] + hi[k];
            cmax = max(cmax, max(lo[k], hi[k]));
            tl[k] = lds.table[lo[k] & (kLdsTable - 1)];
            th[k] = lds.table[hi[k] & (kLdsTable - 1)];
        }
        if (__builtin_expect(cmax >= (uint32_t)kLdsTable, 0)) {
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                if (lo[k] >= (uint32_t)kLdsTable) tl[k] = cover_term(lo[k], len);
                if (hi[k] >= (uint32_t)kLdsTable) th[k] = cover_term(hi[k], len);
            }
        }
        rsum = row_sum_16(rsum);
        if (!ZERO0) wave_total += rsum;
        const float x = row_tree_16(lane_tree_16(tl, th));
        if (i == 0) {
            lds.hist_render[d1] = rsum;
            lds.joint_row_sums[d1] = x;
        }
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int q = (i + 16 * (k + o)) & 127;
        atomicAdd(&lds.hist_warped[q], col_lo[k]);
        atomicAdd(&lds.hist_warped[q + 128], col_hi[k]);
    }
    if (i == 0) atomicAdd(&lds.total[par], wave_total);
}

__device__ __forceinline__ uint32_t popc4(const uint4 &m) { return __popc(m.x) + __popc(m.y) + __popc(m.z) + __popc(m.w); }

// bit 7 of each byte: both mask bytes nonzero (0 elsewhere) -- a mask chunk masked_add_chunk reads as "take"
__device__ __forceinline__ uint4 both_nonzero(const uint4 &a, const uint4 &b)
{
    return {nonzero_byte_bits(a.x) & nonzero_byte_bits(b.x), nonzero_byte_bits(a.y) & nonzero_byte_bits(b.y),
            nonzero_byte_bits(a.z) & nonzero_byte_bits(b.z), nonzero_byte_bits(a.w) & nonzero_byte_bits(b.w)};
}

// Histogram phase of one candidate over all its pixels, all 1024 lanes.  Returns the pixels of this lane whose two masks are
// both nonzero (its share of len).
template <bool BG, bool SHIFTED, int HIST>
__device__ __forceinline__ uint32_t covered_histogram_phase(Lds &lds, int par, const CoveredGridArgs &m, const uint8_t *__restrict__ render,
                                                            const uint8_t *__restrict__ warped, const uint8_t *__restrict__ wmask,
                                                            const uint8_t *__restrict__ rmask, int tid)
{
    const GridArgs &a = m.g;
    uint32_t n = 0;
    if (m.vec_ok) {
        const int nchunks = a.npix >> 4, last = nchunks - 1;
        auto ld = [&](const uint8_t *base, int c) { return *reinterpret_cast<const uint4 *>(base + ((uint32_t)c << 4)); };
        // NMI.cu:82: row y of the frame meets row H-1-y of a bottom-up render -- and of its coverage mask
        auto ldr = [&](const uint8_t *base, int c) {
            const int y = (int)__umulhi((uint32_t)c, a.cpr_magic);
            return *reinterpret_cast<const uint4 *>(base + ((uint32_t)(__mul24(y, a.flip_row) + c + a.flip_base) << 4));
        };
        if (HIST == 1) {
            // exact path (cold): no prefetch
#pragma unroll 1
            for (int ch = tid; ch < nchunks; ch += kBlock) {
                const uint4 cm = both_nonzero(ld(wmask, ch), ldr(rmask, ch));
                n += popc4(cm);
                masked_add_chunk<BG, SHIFTED, HIST>(lds, par, ldr(render, ch), ld(warped, ch), cm, a.shift);
            }
            return n;
        }
        // one chunk of prefetch; loads clamped to the last chunk (a valid address), only the adds are predicated
        int c = min(tid, last);
        uint4 wc = ld(warped, c), rc = ldr(render, c), mc = both_nonzero(ld(wmask, c), ldr(rmask, c));
#pragma unroll 1
        for (int ch = tid; ch < nchunks; ch += kBlock) {
            const int cn = min(ch + kBlock, last);
            const uint4 wn = ld(warped, cn), rn = ldr(render, cn), wmn = ld(wmask, cn), rmn = ldr(rmask, cn);
            n += popc4(mc);
            masked_add_chunk<BG, SHIFTED, HIST>(lds, par, rc, wc, mc, a.shift);
            wc = wn;
            rc = rn;
            mc = both_nonzero(wmn, rmn);
        }
    } else {
        // any width / alignment: byte loads, positions as in NMI.cu:79-83
        for (int pos = tid; pos < a.npix; pos += kBlock) {
            if (wmask[pos] == 0) continue;
            const int y = pos / a.width;
            const int x = pos - y * a.width;
            const int rpos = (a.flip ? (a.height - 1 - y) : y) * a.width + x;
            if (rmask[rpos] == 0) continue;
            ++n;
            uint32_t d1 = render[rpos], d2 = warped[pos];
            if (HIST == 2) {
                if (BG || (d1 != 0 && d2 != 0)) {
                    if (SHIFTED) {
                        d1 >>= a.shift;
                        d2 >>= a.shift;
                    }
                    (void)__hip_atomic_fetch_add(&lds.joint[joint_word(d1, d2)], joint_inc(d2), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
            } else {
                add_pixel<BG, SHIFTED>(lds, par, d1, d2, a.shift);
            }
        }
    }
    return n;
}

// final_phase (nmi_kernels.hip) with the candidate's terms: lds.table for counts below kLdsTable, evaluated above.
__device__ __forceinline__ void covered_final_phase(Lds &lds, const GridArgs &a, uint32_t len, int lane, int p, int w, int s,
                                                    unsigned long long &prev_key)
{
    const int i = lane & 15, r = lane >> 4;
    float lo[8], hi[8];
    // (the counts are read again for the rare evaluation rather than kept: wavefront 0 is at the kernel's register cap here)
    const uint32_t *h = r == 0 ? lds.hist_render : lds.hist_warped;
    uint32_t cmax = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const uint32_t cl = r < 2 ? h[i + 16 * k] : 0u, ch = r < 2 ? h[i + 16 * k + 128] : 0u;
        cmax = max(cmax, max(cl, ch));
        lo[k] = lds.table[cl & (kLdsTable - 1)];
        hi[k] = lds.table[ch & (kLdsTable - 1)];
    }
    if (__builtin_expect(cmax >= (uint32_t)kLdsTable, 0)) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const uint32_t cl = h[i + 16 * k], ch = h[i + 16 * k + 128];  // (only rows 0 and 1 can get here)
            if (cl >= (uint32_t)kLdsTable) lo[k] = cover_term(cl, len);
            if (ch >= (uint32_t)kLdsTable) hi[k] = cover_term(ch, len);
        }
    }
    if (r == 2) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            lo[k] = lds.joint_row_sums[i + 16 * k];
            hi[k] = lds.joint_row_sums[i + 16 * k + 128];
        }
    }
    const float x = row_tree_16(lane_tree_16(lo, hi));
    const float a1 = __shfl(x, 0, 64), a2 = __shfl(x, 16, 64), a3 = __shfl(x, 32, 64);
    if (lane == 0) commit_score(a, p, w, s, a1, a2, a3, prev_key);
}

}  // namespace

#ifndef NMI_COVERED_DEVICE_ONLY
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
        {
            uint4 *j4 = reinterpret_cast<uint4 *>(lds.joint);
            const uint4 z = {0, 0, 0, 0};
            for (int i = tid; i < kWords / 4; i += kBlock) j4[i] = z;
        }
        if (tid < kBins) lds.hist_warped[tid] = 0;
        if (tid < 2) lds.ovf_n[tid] = lds.total[tid] = 0;
        if (tid < 2 * kSide) (&lds.side_key[0][0])[tid] = (&lds.side_cnt[0][0])[tid] = 0;  // never set here; the decode reads them
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
                if (lane == 0) m.redo[__hip_atomic_fetch_add(m.redo_n, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)] = p;
            } else {
                covered_final_phase(lds, a, len, lane, p, w, s, prev_key);
            }
            for (int t = lane; t < kBins; t += 64) lds.hist_warped[t] = 0;
            if (lane == 0) {
                lds.ovf_n[par] = 0;      // consumed by this candidate's decode; next used two candidates on
                lds.total[par ^ 1] = 0;  // read by everyone right after the previous B2; next candidate adds to it
            }
        }
    }

    if (wave == 0) {
        if (from_list && lane == 0) {
            // the list is consumed: the workgroup that arrives last (everyone has read the count) leaves it empty
            if (__hip_atomic_fetch_add(m.redo_done, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1) {
                __hip_atomic_store(m.redo_n, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(m.redo_done, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        finish_search(a, lane, prev_key, gridDim.x);
    }
}

template <bool BG, bool SHIFTED>
static void launch_covered_pair(const CoveredGridArgs &m, int workgroups, bool exact, hipStream_t stream)
{
    const dim3 grid(workgroups), block(kBlock);
    if (exact) {
        CoveredGridArgs e = m;
        e.redo = nullptr;
        hipLaunchKernelGGL((nmi_covered_grid_kernel<BG, SHIFTED, 1>), grid, block, 0, stream, e);
        return;
    }
    CoveredGridArgs o = m;  // the optimistic launch publishes nothing; the exact one after it does
    o.g.mailbox = nullptr;
    o.g.out_key = nullptr;
    o.g.score_post = nullptr;
    hipLaunchKernelGGL((nmi_covered_grid_kernel<BG, SHIFTED, 3>), grid, block, 0, stream, o);
    if (hipPeekAtLastError() != hipSuccess) return;
    hipLaunchKernelGGL((nmi_covered_grid_kernel<BG, SHIFTED, 1>), grid, block, 0, stream, m);
}

hipError_t launch_grid_covered(const CoveredGridArgs &m, int workgroups, bool use_bg, bool exact, hipStream_t stream)
{
    const bool shifted = m.g.shift != 0;
    exact = exact || (!use_bg && shifted);  // BG off below 256 bins: the rule looks at raw values, bin 0 also holds 1 .. 2^shift - 1
    if (m.g.plan || !m.counts || (!exact && (!m.redo || !m.redo_n || !m.redo_done))) return hipErrorInvalidValue;
    if (use_bg) {
        if (shifted) launch_covered_pair<true, true>(m, workgroups, exact, stream);
        else launch_covered_pair<true, false>(m, workgroups, exact, stream);
    } else {
        if (shifted) launch_covered_pair<false, true>(m, workgroups, exact, stream);
        else launch_covered_pair<false, false>(m, workgroups, exact, stream);
    }
    return hipGetLastError();
}
#endif  // !NMI_COVERED_DEVICE_ONLY

}  // namespace nmi
