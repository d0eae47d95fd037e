// nmi_masked_kernel.hip -- the masked grid search: nmi_grid_kernel's computation with a per-warp pixel mask.
//
// A candidate (warp w, render s) counts pixel pos iff mask[w][pos] != 0 and the background rule passes (NMI.cu:85, on the
// raw intensities, before the shift); the entropy terms use len_w = popcount(mask[w]) in place of W*H (NMI.cu:245), so each
// warp has its own per-count table.  Everything else -- the trees, SUC / ENMI, the all-zero guard, the rating table and the
// arg-max -- is nmi_grid_kernel's own code (nmi_kernels.hip, included below for its device functions only; the existing
// kernels' translation units are untouched).
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

// nmi_masked_pix_kernel.hip includes this file for its device functions only (NMI_MASKED_DEVICE_ONLY), after nmi_kernels.hip.
#ifndef NMI_MASKED_DEVICE_ONLY
#define NMI_KERNELS_DEVICE_ONLY 1
#include "nmi_kernels.hip"  // Lds, add_chunk, add_pixel, decode_phase, final_phase, finish_search, candidate_at
#endif
#include "nmi_masked.h"

namespace nmi {

namespace {

// number of nonzero bytes of a dword (bit 7 of each byte of the sum is set iff the byte is nonzero)
__device__ __forceinline__ uint32_t nonzero_byte_bits(uint32_t v) { return (((v & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | v) & 0x80808080u; }

// 16 pixels of one lane with their 16 mask bytes.  HIST 2: non-returning atomics (optimistic pass); a wavefront whose mask
// bytes are all nonzero runs add_chunk (nmi_kernels.hip) unchanged.  The choice is per wavefront, not per lane: an LDS atomic
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

}  // namespace

#ifndef NMI_MASKED_DEVICE_ONLY
// One workgroup per candidate, grid-stride over the candidates in the visiting order -- nmi_grid_kernel's structure: B1
// histogram -> decode, B2 decode -> (wavefront 0: final trees + score + arg-max) || (the others: next candidate's pixels),
// per-candidate state double-buffered by parity.
//   HIST 3: optimistic pass (non-returning atomics) and the count test.  A candidate that fails it is not scored: it is
//           appended to m.redo, and the HIST 1 launch that follows (m.redo set there too) scores it exactly.  nmi_grid_kernel
//           redoes such candidates in a cold loop of its own; here that loop pushed the kernel past its 128 VGPRs into
//           scratch, the second launch does not (and costs one launch that returns at once when nothing failed).
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
        {
            uint4 *j4 = reinterpret_cast<uint4 *>(lds.joint);
            const uint4 z = {0, 0, 0, 0};
            for (int i = tid; i < kWords / 4; i += kBlock) j4[i] = z;
        }
        if (tid < kBins) lds.hist_warped[tid] = 0;
        if (tid < 2) lds.ovf_n[tid] = lds.total[tid] = 0;
        if (tid < 2 * kSide) (&lds.side_key[0][0])[tid] = (&lds.side_cnt[0][0])[tid] = 0;  // never set here; decode_phase reads them
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
                if (lane == 0) m.redo[__hip_atomic_fetch_add(m.redo_n, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)] = p;
            } else {
                final_phase(lds, aw, lane, p, w, s, prev_key);
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

template <bool BG, bool SHIFTED>
static void launch_masked_pair(const MaskedGridArgs &m, int workgroups, bool exact, hipStream_t stream)
{
    const dim3 grid(workgroups), block(kBlock);
    if (exact) {
        MaskedGridArgs e = m;
        e.redo = nullptr;
        hipLaunchKernelGGL((nmi_masked_grid_kernel<BG, SHIFTED, 1>), grid, block, 0, stream, e);
        return;
    }
    MaskedGridArgs o = m;  // the optimistic launch publishes nothing; the exact one after it does
    o.g.mailbox = nullptr;
    o.g.out_key = nullptr;
    o.g.score_post = nullptr;
    hipLaunchKernelGGL((nmi_masked_grid_kernel<BG, SHIFTED, 3>), grid, block, 0, stream, o);
    if (hipPeekAtLastError() != hipSuccess) return;
    hipLaunchKernelGGL((nmi_masked_grid_kernel<BG, SHIFTED, 1>), grid, block, 0, stream, m);
}

hipError_t launch_grid_masked(const MaskedGridArgs &m, int workgroups, bool use_bg, bool exact, hipStream_t stream)
{
    const bool shifted = m.g.shift != 0;
    exact = exact || (!use_bg && shifted);  // BG off below 256 bins: the rule looks at raw values, bin 0 also holds 1 .. 2^shift - 1
    if (m.g.plan || (!exact && (!m.redo || !m.redo_n || !m.redo_done))) return hipErrorInvalidValue;
    if (use_bg) {
        if (shifted) launch_masked_pair<true, true>(m, workgroups, exact, stream);
        else launch_masked_pair<true, false>(m, workgroups, exact, stream);
    } else {
        if (shifted) launch_masked_pair<false, true>(m, workgroups, exact, stream);
        else launch_masked_pair<false, false>(m, workgroups, exact, stream);
    }
    return hipGetLastError();
}
#endif  // !NMI_MASKED_DEVICE_ONLY

}  // namespace nmi
