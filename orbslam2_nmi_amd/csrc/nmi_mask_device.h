// nmi_mask_device.h -- device code of the masked and covered searches (nmi_masked_kernel.hip, nmi_covered_kernel.hip,
// their pixel-range forms and nmi_masked_level.hip): the masked chunk and pixel forms, the mask fold of the covered search,
// its per-candidate terms and its decode / final trees, and what the masked and the covered grid kernel do alike around their
// redo list (redo_append, redo_consumed, the launch pair).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nmi_grid_device.h"
#include "nmi_masked.h"
#include "nmi_covered.h"

namespace nmi {

namespace {

// number of nonzero bytes of a dword (bit 7 of each byte of the sum is set iff the byte is nonzero)
__device__ __forceinline__ uint32_t nonzero_byte_bits(uint32_t v) { return (((v & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | v) & 0x80808080u; }

// 16 pixels of one lane with their 16 mask bytes.  HIST 2: non-returning atomics (optimistic pass); a wavefront whose mask
// bytes are all nonzero runs add_chunk (nmi_grid_device.h) unchanged.  The choice is per wavefront, not per lane: an LDS atomic
// costs its issue whatever the number of active lanes, so a wavefront that ran both forms for its lanes would issue 32 atomic
// instructions per 16 pixels (measured: 1.4x the kernel time with the border masks of a rotation grid).  HIST 1: returning
// atomics + wrap bookkeeping (exact path), in batches of 4 pixels -- 4 returned words in flight instead of add_chunk's 16
// keep this cold path inside the register budget.
template <bool BG, bool SHIFTED, int HIST>
__device__ __forceinline__ void masked_add_chunk(Lds &lds, int par, const uint4 &rv, const uint4 &wv, const uint4 &mv, int shift)
{
    if (HIST == 2 &&
        __all((nonzero_byte_bits(mv.x) & nonzero_byte_bits(mv.y) & nonzero_byte_bits(mv.z) & nonzero_byte_bits(mv.w)) == 0x80808080u)) {
        add_chunk<BG, SHIFTED, HIST, false>(lds, par, rv, wv, shift, false);  // every pixel takes part
        return;
    }
    const uint32_t r[4] = {rv.x, rv.y, rv.z, rv.w};
    const uint32_t w[4] = {wv.x, wv.y, wv.z, wv.w};
    const uint32_t m[4] = {mv.x, mv.y, mv.z, mv.w};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        uint32_t old[4], any = 0;  // any: 0xFFFFFFFF iff some counter wrapped (a pixel that was not added has old = 0)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            uint32_t d1 = (r[q] >> (8 * j)) & 0xFFu, d2 = (w[q] >> (8 * j)) & 0xFFu;
            const bool take = ((m[q] >> (8 * j)) & 0xFFu) != 0u && (BG || (d1 != 0 && d2 != 0));  // NMI.cu:85 on the raw values
            if (SHIFTED) {
                d1 >>= shift;
                d2 >>= shift;
            }
            const uint32_t word = joint_word(d1, d2), val = joint_inc(d2);
            if (HIST == 2) {
                if (take) (void)__hip_atomic_fetch_add(&lds.joint[word], val, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            } else {
                old[j] = 0;
                if (take) old[j] = __hip_atomic_fetch_add(&lds.joint[word], val, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
        }
        if (HIST == 1) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                uint32_t d2 = (w[q] >> (8 * j)) & 0xFFu;
                if (SHIFTED) d2 >>= shift;
                const uint32_t t = old[j] | ((d2 & 128u) ? 0x0000FFFFu : 0xFFFF0000u);
                any = t > any ? t : any;
            }
            if (__builtin_expect(any == 0xFFFFFFFFu, 0)) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    uint32_t d1 = (r[q] >> (8 * j)) & 0xFFu, d2 = (w[q] >> (8 * j)) & 0xFFu;
                    const bool take = ((m[q] >> (8 * j)) & 0xFFu) != 0u && (BG || (d1 != 0 && d2 != 0));
                    if (SHIFTED) {
                        d1 >>= shift;
                        d2 >>= shift;
                    }
                    const uint32_t val = joint_inc(d2), field = val * 0xFFFFu;
                    if (take && (old[j] & field) == field) record_wrap(lds, par, joint_word(d1, d2), val, old[j]);
                }
            }
        }
    }
}

// Histogram phase of one candidate over all its pixels (NMI.cu:79-87 with the mask), all 1024 lanes.
template <bool BG, bool SHIFTED, int HIST>
__device__ __forceinline__ void masked_histogram_phase(Lds &lds, int par, const MaskedGridArgs &m, const uint8_t *__restrict__ render,
                                                       const uint8_t *__restrict__ warped, const uint8_t *__restrict__ mask, int tid)
{
    const GridArgs &a = m.g;
    if (m.vec_ok) {
        const int nchunks = a.npix >> 4, last = nchunks - 1;
        auto ld = [&](const uint8_t *base, int c) { return *reinterpret_cast<const uint4 *>(base + ((uint32_t)c << 4)); };
        // NMI.cu:82: row y of the frame meets row H-1-y of a bottom-up render (flip_base / flip_row, as histogram_phase)
        auto ldr = [&](int c) {
            const int y = (int)__umulhi((uint32_t)c, a.cpr_magic);
            return *reinterpret_cast<const uint4 *>(render + ((uint32_t)(__mul24(y, a.flip_row) + c + a.flip_base) << 4));
        };
        if (HIST == 1) {
            // exact path (cold): no prefetch -- the 16 returned words of a chunk already hold 16 registers
#pragma unroll 1
            for (int ch = tid; ch < nchunks; ch += kBlock) masked_add_chunk<BG, SHIFTED, HIST>(lds, par, ldr(ch), ld(warped, ch), ld(mask, ch), a.shift);
            return;
        }
        // one chunk of prefetch; loads clamped to the last chunk (a valid address), only the adds are predicated
        int c = min(tid, last);
        uint4 wc = ld(warped, c), mc = ld(mask, c), rc = ldr(c);
#pragma unroll 1
        for (int ch = tid; ch < nchunks; ch += kBlock) {
            const int cn = min(ch + kBlock, last);
            const uint4 wn = ld(warped, cn), mn = ld(mask, cn), rn = ldr(cn);
            masked_add_chunk<BG, SHIFTED, HIST>(lds, par, rc, wc, mc, a.shift);
            wc = wn;
            mc = mn;
            rc = rn;
        }
    } else {
        // any width / alignment: byte loads, positions as in NMI.cu:79-83
        for (int pos = tid; pos < a.npix; pos += kBlock) {
            if (mask[pos] == 0) continue;
            const int y = pos / a.width;
            const int x = pos - y * a.width;
            const int ry = a.flip ? (a.height - 1 - y) : y;
            uint32_t d1 = render[ry * a.width + x], d2 = warped[pos];
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
}


// term of count c for len pixels: nmi_table_kernel's / nmi_mask_table_kernel's expression, bit for bit
__device__ __forceinline__ float cover_term(uint32_t c, uint32_t len)
{
    if (c == 0u) return 0.0f;
    const float p = (float)c / (float)len;
    const float l = (float)log2((double)p);
    return p * l;
}

// ---- decode phase: decode_phase (nmi_grid_device.h) with the candidate's terms -------------------------------------------------
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
    const int i = lane & 15, r = lane >> 4;
    uint32_t col_lo[8], col_hi[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) col_lo[k] = col_hi[k] = 0;
#pragma unroll 1
    for (int pass = 0; pass < kRowsPerWave / 4; ++pass) {
        const int d1 = decode_row(wave, pass, r);
        const uint32_t a0 = decode_word(d1, i, 0);
        uint32_t lo[8], hi[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const uint32_t idx = a0 + 16 * k;
            const uint32_t wd = lds.joint[idx];
            lds.joint[idx] = 0;  // ready for the next candidate
            lo[k] = wd & 0xFFFFu;
            hi[k] = wd >> 16;
        }
        if (__builtin_expect(novf != 0, 0)) {
#pragma unroll
            for (int k = 0; k < 8; ++k) apply_wraps(lds, par, novf, a0 + 16 * k, lo[k], hi[k]);
        }
        uint32_t rsum = 0, cmax = 0;
        if (ZERO0) {
            uint32_t raw = 0;
#pragma unroll
            for (int k = 0; k < 8; ++k) raw += lo[k] + hi[k];
            wave_total += row_sum_16(raw);
            if (i == 0) lo[0] = 0;  // the bin d2 = 0 of this row
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
        const int q = i + 16 * k;
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

// final_phase (nmi_grid_device.h) with the candidate's terms: lds.table for counts below kLdsTable, evaluated above.
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

// ---- the redo list of the masked and the covered grid kernel (M: MaskedGridArgs / CoveredGridArgs) ---------------------------
// The optimistic launch (HIST 3) appends the candidates that failed its count test to m.redo; the exact launch (HIST 1) that
// follows it scores them and leaves the list empty (why two launches: nmi_masked_kernel.hip).
// One lane, optimistic launch: candidate p is left to the exact launch.
template <class M>
__device__ __forceinline__ void redo_append(const M &m, int p)
{
    m.redo[__hip_atomic_fetch_add(m.redo_n, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)] = p;
}
// One lane of every workgroup of an exact launch that read the list, at its end: the list is consumed, and the workgroup that
// arrives last (everyone has read the count) leaves it empty.
template <class M>
__device__ __forceinline__ void redo_consumed(const M &m)
{
    if (__hip_atomic_fetch_add(m.redo_done, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1) {
        __hip_atomic_store(m.redo_n, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(m.redo_done, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}
// Host: a search as the pair of launches -- optimistic, then exact over the list -- or, `exact`, as one exact launch over the grid.
template <class M>
static void launch_redo_pair(void (*optimistic_kernel)(M), void (*exact_kernel)(M), const M &m, int workgroups, bool exact, hipStream_t stream)
{
    const dim3 grid(workgroups), block(kBlock);
    if (exact) {
        M e = m;
        e.redo = nullptr;
        hipLaunchKernelGGL(exact_kernel, grid, block, 0, stream, e);
        return;
    }
    M o = m;  // the optimistic launch publishes nothing; the exact one after it does
    o.g.mailbox = nullptr;
    o.g.out_key = nullptr;
    o.g.score_post = nullptr;
    hipLaunchKernelGGL(optimistic_kernel, grid, block, 0, stream, o);
    if (hipPeekAtLastError() != hipSuccess) return;
    hipLaunchKernelGGL(exact_kernel, grid, block, 0, stream, m);
}

}  // namespace

}  // namespace nmi
