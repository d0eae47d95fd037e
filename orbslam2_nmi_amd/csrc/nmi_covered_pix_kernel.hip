// nmi_covered_pix_kernel.hip -- the covered search for MID-SIZE grids (33 ... 128 candidates on 256 compute units, and the
// grids choose_pix sends here on frames whose rows are not whole aligned chunks): nmi_pix_kernel's pixel ranges (P workgroups
// per candidate, an owner and P - 1 helpers, dealt pieces of the frame) with nmi_covered_grid_kernel's masks on both sides and
// per-candidate len.  nmi_covered_grid_kernel gives a candidate to one workgroup, so 81 candidates fill 81 of the 256 CUs;
// here they fill 243.
//
// Restated: covered_decode_merged, decode_merged with the candidate's terms (see TWIN there), and the hand-off (a TWIN of
// nmi_pix_kernel's).  Reused: the dealing (make_deal, pix_dealing) and the hand-off blocks (PixHeader, unit layout, tagged
// mask granules) from nmi_pix_device.h; masked_add_chunk, the mask fold (both_nonzero), the term expression (cover_term), the
// exact path (covered_histogram_phase, covered_decode_phase) and the final trees (covered_final_phase) from
// nmi_mask_device.h.  Results are bit-identical to nmi_covered_grid_kernel's: the decoded counters are the same sums,
// the trees the same code, the terms the same expression of the same len.
//
// What differs from nmi_masked_pix_kernel, and why:
//   * len from the ranges.  Each workgroup counts the pixels of its range whose two mask bytes are both nonzero; a helper hands
//     that count over in its block's header (stored before the drain that precedes its tagged granules, so an owner that sees
//     a tag has it), and the owner sums all ranges.  That sum is len[w][s], and it serves twice: as the expected decoded total
//     of the count test (a wrapped 16-bit field always loses weight, so the decoded sum falls short iff something wrapped) and
//     as the terms' denominator.  The two are the same number only because every covered pixel is added -- the background
//     rule on, or off at 256 bins (row / column 0 cleared in the decode).  The background rule off with fewer than 256 bins
//     drops pixels by their raw values, which would make them differ; choose_pix never sends that case to a pixel-range kernel.
//   * Terms.  Known only once every hand-off has arrived: the owner then evaluates the low terms (c <= min(len, kLdsTable - 1))
//     into lds.table with cover_term, and counts at or above kLdsTable are evaluated inline during the merged decode and the
//     final trees, as covered_decode_phase does.  No global table is read.
//   * Outputs.  The owner writes counts[w][s] (nmi_last_cover_counts), the rating, and posts the winner like
//     launch_grid_covered.
//   * Heal.  A candidate that fails the count test, or whose helper did not arrive within the bounded wait, is scored by its
//     owner alone on the covered exact path (covered_histogram_phase with returning atomics + wrap bookkeeping,
//     covered_decode_phase, covered_final_phase) inside the launch; both are counted in *healed (nmi_pix_status().healed).
//   * Shapes.  Rows need not be whole aligned chunks: the dealt chunks take nmi_pix_kernel's unaligned-row addressing for the
//     frame, the render and both masks alike (the render mask in the render's row order), and the owner adds the rows' last
//     width % 16 pixels one by one (frames of at least 32 pixels of width, e.g. 1241 x 376).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nmi_mask_device.h"  // masked_add_chunk, cover_term, both_nonzero, popc4, covered_histogram_phase, covered_decode_phase, covered_final_phase
#include "nmi_pix_device.h"   // Deal, make_deal, PixHeader, decode_word, unit_offset

namespace nmi {

namespace {

// This workgroup's dealt pieces (histogram_dealt's addressing, nmi_pix_kernel.hip) with both masks folded, non-returning
// atomics.  Returns the pixels this lane added (its share of len).
template <bool SHIFTED>
__device__ __forceinline__ uint32_t covered_histogram_dealt(Lds &lds, const GridArgs &a, const uint8_t *__restrict__ render,
                                                           const uint8_t *__restrict__ warped, const uint8_t *__restrict__ wmask,
                                                           const uint8_t *__restrict__ rmask, int wave, int lane, const Deal &d)
{
    const int nchunks = a.height * a.chunks_per_row, last = nchunks - 1, row_rem = a.width - (a.chunks_per_row << 4);
    auto at = [&](int c) {  // byte of chunk c in the frame (and in the warp mask: same layout)
        c = min(c, last);
        return ((uint32_t)c << 4) + (uint32_t)__mul24((int)__umulhi((uint32_t)c, a.cpr_magic), row_rem);
    };
    auto rat = [&](int c) {  // byte of chunk c in the render (and in its coverage mask): NMI.cu:82, row y meets row H-1-y
        c = min(c, last);
        const int y = (int)__umulhi((uint32_t)c, a.cpr_magic);
        const int ry = a.flip ? a.height - 1 - y : y;
        return ((uint32_t)(__mul24(y, a.flip_row) + c + a.flip_base) << 4) + (uint32_t)__mul24(ry, row_rem);
    };
    auto chunk_of = [&](int it) {
        const int i = it * kWaves + wave;  // wavefront-uniform
        const int g = d.cnt > 1 ? (int)__umulhi((uint32_t)i, d.magic) : i;
        const int t = g * d.L + d.off + (i - g * d.cnt);
        return i < d.n ? (t << 6) + lane : 0x7FFFFFC0;
    };
    auto ld = [](const uint8_t *base, uint32_t o) { return *reinterpret_cast<const uint4 *>(base + o); };
    uint32_t added = 0;
    if (d.off == 0 && row_rem > 0) {
        // the owner also adds the last width % 16 pixels of every row
        const int x0 = a.chunks_per_row << 4, n = a.height * row_rem;
        for (int t = wave * 64 + lane; t < n; t += kBlock) {
            const int y = t / row_rem, x = x0 + t - y * row_rem;
            const int rpos = (a.flip ? a.height - 1 - y : y) * a.width + x;
            if (wmask[y * a.width + x] == 0 || rmask[rpos] == 0) continue;
            uint32_t d1 = render[rpos], d2 = warped[y * a.width + x];
            if (SHIFTED) {
                d1 >>= a.shift;
                d2 >>= a.shift;
            }
            (void)__hip_atomic_fetch_add(&lds.joint[joint_word(d1, d2)], joint_inc(d2), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            ++added;
        }
    }
    const int iters = (d.n + kWaves - 1) / kWaves;  // workgroup-uniform
    if (iters <= 0) return added;
    // one chunk of prefetch (covered_histogram_phase's loop); loads clamped to the last chunk, only the adds are predicated
    int c = chunk_of(0);
    uint32_t o = at(c), ro = rat(c);
    uint4 wc = ld(warped, o), rc = ld(render, ro), mc = both_nonzero(ld(wmask, o), ld(rmask, ro));
#pragma unroll 1
    for (int it = 0; it < iters; ++it) {
        const int cn = chunk_of(it + 1);
        const uint32_t on = at(cn), rn_o = rat(cn);
        const uint4 wn = ld(warped, on), rn = ld(render, rn_o), wmn = ld(wmask, on), rmn = ld(rmask, rn_o);
        if (c < nchunks) {
            added += popc4(mc);
            masked_add_chunk<true, SHIFTED, 2>(lds, 0, rc, wc, mc, a.shift);
        }
        wc = wn;
        rc = rn;
        mc = both_nonzero(wmn, rmn);
        c = cn;
    }
    return added;
}

// the workgroup's added pixels into *dst (LDS, zero before)
__device__ __forceinline__ void add_cover_count(uint32_t *dst, uint32_t n, int lane)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) n += (uint32_t)__shfl_xor((int)n, off, 64);
    if (lane == 0) atomicAdd(dst, n);
}

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

// The owner's decode: decode_merged (nmi_pix_kernel.hip) over its own packed counters plus the helpers' (acc), with the
// candidate's terms -- lds.table below kLdsTable, cover_term above, as covered_decode_phase.  Left out, as there: the side
// counters (the masked pixel forms never fold flat chunks) and the debug copy.
// TWIN: a copy of decode_merged (nmi_pix_kernel.hip), line for line apart from the high-count terms and the two left-out parts
// -- a fix to one belongs in the other.  A copy because decode_merged's code may not change (its kernels' assembly stays as
// it is) and its high-count branch reads a global table this kernel does not have.
template <bool ZERO0>
__device__ __forceinline__ void covered_decode_merged(Lds &lds, uint32_t len, int wave, int lane, const u32x4 (&acc)[kUnitsPerLane])
{
    uint32_t wave_total = 0;
    const int i = lane & 15, r = lane >> 4;
    uint32_t col_lo[8], col_hi[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) col_lo[k] = col_hi[k] = 0;
#pragma unroll
    for (int pass = 0; pass < kRowsPerWave / 4; ++pass) {
        const int d1 = decode_row(wave, pass, r);
        uint32_t lo[8], hi[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const uint32_t wd = lds.joint[decode_word(d1, i, k)];
            const uint32_t ad = acc[pass * 2 + (k >> 2)][k & 3];
            lo[k] = (wd & 0xFFFFu) + (ad & 0xFFFFu);
            hi[k] = (wd >> 16) + (ad >> 16);
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
    if (i == 0) atomicAdd(&lds.total[0], wave_total);
}

}  // namespace

// Workgroup b: helpers first (blocks 0 .. total * (P - 1) - 1: range q = 1 + b / total of candidate b % total), then the owners
// -- nmi_pix_kernel's liveness argument unchanged.  ZERO0: background rule off at 256 bins (row / column 0 cleared in the decode).
template <bool ZERO0, bool SHIFTED>
__global__ __launch_bounds__(NMI_BLOCK_THREADS) void nmi_covered_pix_kernel(CoveredGridArgs m, int P, DealArgs dealing, const uint32_t *replay,
                                                                           uint32_t *healed)
{
    __shared__ Lds lds;
    const GridArgs &a = m.g;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;

    const int total = a.S_local * a.Wn;
    const int helpers = total * (P - 1);
    const int b = (int)blockIdx.x;
    const int q = b < helpers ? 1 + (total > 1 ? (int)__umulhi((uint32_t)b, dealing.total_magic) : b) : 0;
    const int p = b < helpers ? b - (q - 1) * total : b - helpers;
    const bool owner = q == 0;
    const int w = p / a.S_local, s = p - w * a.S_local;
    const uint8_t *render = a.render_stack + (size_t)s * a.npix;
    const uint8_t *warped = a.warp_stack + (size_t)w * a.npix;
    const uint8_t *wmask = m.warp_masks + (size_t)w * a.npix;
    const uint8_t *rmask = m.render_masks + (size_t)s * a.npix;
    const uint32_t tag = 0x80000000u | ((a.epoch + (replay ? __hip_atomic_load(replay, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u)) & 0x7FFFFFFFu);

    if (b == 0 && tid == 0 && a.reset_key) *a.reset_key = 0ull;  // next launch's slot; idle during this one
    {
        uint4 *j4 = reinterpret_cast<uint4 *>(lds.joint);
        const uint4 z = {0, 0, 0, 0};
        for (int i = tid; i < kJointWords / 4; i += kBlock) j4[i] = z;
    }
    if (tid < kBins) lds.hist_warped[tid] = 0;
    if (tid < 2) lds.ovf_n[tid] = lds.total[tid] = 0;  // total[0]: decoded counters, total[1]: len (pixels added by all ranges)
    if (tid < 2 * kSide) (&lds.side_key[0][0])[tid] = (&lds.side_cnt[0][0])[tid] = 0;  // never set here; the exact decode reads none
    if (tid == 0) lds.fallback = 0;
    const Deal deal = make_deal(dealing, P, q);
    __syncthreads();
    add_cover_count(&lds.total[1], covered_histogram_dealt<SHIFTED>(lds, a, render, warped, wmask, rmask, wave, lane, deal), lane);

    char *const blocks = reinterpret_cast<char *>(a.blocks) + (size_t)p * (size_t)(P - 1) * kPixBlockBytes;
    if (!owner) {
        // ---- helper: nmi_pix_kernel's hand-off, plus the count of pixels added (header word pad[0]) ----
        // TWIN: nmi_pix_kernel's helper part and owner's wait and merge, written out (see there) -- a fix there belongs here too.
        __syncthreads();
        char *const blk = blocks + (size_t)(q - 1) * kPixBlockBytes;
        PixHeader *const hdr = reinterpret_cast<PixHeader *>(blk);
        const auto rsrc = __builtin_amdgcn_make_buffer_rsrc(blk, 0, (int)kPixBlockBytes, 0x00020000);
        unsigned long long bits[kUnitsPerLane];
        {
            const int i = lane & 15, r = lane >> 4;
#pragma unroll
            for (int kk = 0; kk < kUnitsPerLane; ++kk) {
                const int d1 = decode_row(wave, kk >> 1, r);
                u32x4 v;
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = lds.joint[decode_word(d1, i, (kk & 1) * 4 + j)];
                const bool on = (v.x | v.y | v.z | v.w) != 0u;
                bits[kk] = __ballot(on);
                if (on) __builtin_amdgcn_raw_buffer_store_b128(v, rsrc, unit_offset(wave, kk, lane), 0, kAuxSc1);
            }
        }
        if (tid == 0) __hip_atomic_store(&hdr->pad[0], lds.total[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        uint32_t half = 0;
#pragma unroll
        for (int g = 0; g < 2 * kUnitsPerLane; ++g)
            if (lane == g) half = (uint32_t)(bits[g >> 1] >> (32 * (g & 1)));
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every storing wave, before the barrier the granules' lanes wait at
        __syncthreads();
        // (phase mask bit 9, tests only: helper 1 keeps its masks to itself, so its owner's wait must time out and heal)
        if (lane < 2 * kUnitsPerLane && !((a.phase_mask & 512) && q == 1))
            __hip_atomic_store(&hdr->granule[wave * 2 * kUnitsPerLane + lane], ((unsigned long long)tag << 32) | half, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;
    }

    // ---- owner ----
    unsigned long long gv = 0;
    bool seen = true;
    if (lane < 16 * (P - 1)) {
        const unsigned long long *g = reinterpret_cast<const PixHeader *>(blocks + (size_t)(lane >> 4) * kPixBlockBytes)->granule + wave * 16 + (lane & 15);
        unsigned long long t0 = 0;
        int tries = 0;
        while ((uint32_t)((gv = __hip_atomic_load(g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) >> 32) != tag) {
            __builtin_amdgcn_s_sleep(4);
            if ((++tries & 15) == 1) {
                const unsigned long long now = wall_clock64();
                if (tries == 1) t0 = now;
                if (now - t0 > kPixTimeoutTicks || tries > (1 << 20)) {
                    seen = false;
                    break;
                }
            }
        }
    }
    seen = __all(seen);  // wave-uniform
    if (!seen && lane == 0) lds.fallback = 1;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");  // (no instruction: keeps the loads below behind the poll)
    const uint32_t gh = (uint32_t)gv;
    u32x4 acc[kUnitsPerLane];
#pragma unroll
    for (int kk = 0; kk < kUnitsPerLane; ++kk) acc[kk] = u32x4{0, 0, 0, 0};
    if (seen) {
        for (int h = 0; h < P - 1; ++h) {
            const char *blk = blocks + (size_t)h * kPixBlockBytes;
            const auto rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<char *>(blk), 0, (int)kPixBlockBytes, 0x00020000);
            u32x4 v[kUnitsPerLane];
#pragma unroll
            for (int kk = 0; kk < kUnitsPerLane; ++kk) {
                const uint32_t lo = __builtin_amdgcn_readlane(gh, h * 16 + 2 * kk), hi = __builtin_amdgcn_readlane(gh, h * 16 + 2 * kk + 1);
                v[kk] = u32x4{0, 0, 0, 0};
                if ((((((unsigned long long)hi << 32) | lo) >> lane) & 1ull) != 0ull) v[kk] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, unit_offset(wave, kk, lane), 0, kAuxSc1);
            }
            if (wave == 0 && lane == 0) atomicAdd(&lds.total[1], __builtin_amdgcn_raw_buffer_load_b32(rsrc, (int)offsetof(PixHeader, pad), 0, kAuxSc1));
#pragma unroll
            for (int kk = 0; kk < kUnitsPerLane; ++kk) acc[kk] += v[kk];
        }
    }
    __syncthreads();  // B1: every wavefront's pixels are in the counters, every helper's count in total[1]
    unsigned long long prev_key = 0;
    bool alone = lds.fallback != 0;  // some wave gave up on a helper (workgroup-uniform)
    if (!alone) {
        const uint32_t len = lds.total[1];
        cover_terms(lds, len, tid);
        __syncthreads();  // B1b: the candidate's low terms are in lds.table
        covered_decode_merged<ZERO0>(lds, len, wave, lane, acc);
        __syncthreads();
        alone = lds.total[0] != len;  // some 16-bit field wrapped (workgroup-uniform, rare)
        if (!alone && wave == 0) {
            if (lane == 0) m.counts[p] = (int32_t)len;
            covered_final_phase(lds, a, len, lane, p, w, s, prev_key);
        }
    }
    if (alone) {
        // cold: this candidate once more, by this workgroup alone, on the covered exact path
        if (tid == 0 && healed) __hip_atomic_fetch_add(healed, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();
        {
            uint4 *j4 = reinterpret_cast<uint4 *>(lds.joint);
            const uint4 z = {0, 0, 0, 0};
            for (int i = tid; i < kJointWords / 4; i += kBlock) j4[i] = z;
        }
        if (tid < kBins) lds.hist_warped[tid] = 0;
        if (tid < 2) lds.total[tid] = lds.ovf_n[tid] = 0;
        __syncthreads();
        const uint32_t n = covered_histogram_phase<true, SHIFTED, 1>(lds, 0, m, render, warped, wmask, rmask, tid);
        add_cover_count(&lds.total[1], n, lane);
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
    if (wave == 0) finish_search(a, lane, prev_key, (uint32_t)total);
}

// One launch of total * pix_parts workgroups (nmi_covered.h).
hipError_t launch_pix_covered(const CoveredGridArgs &m, int pix_parts, double owner_share, bool use_bg, const uint32_t *replay, uint32_t *healed,
                              hipStream_t stream)
{
    const GridArgs &a = m.g;
    if (!pix_launch_ok(a, pix_parts, use_bg) || a.plan || !m.counts || !m.warp_masks || !m.render_masks) return hipErrorInvalidValue;
    const long long total = (long long)a.S_local * a.Wn;
    const DealArgs g = pix_dealing(a, pix_parts, owner_share);
    const dim3 grid((unsigned)(total * pix_parts)), block(kBlock);
    if (a.shift != 0)
        hipLaunchKernelGGL((nmi_covered_pix_kernel<false, true>), grid, block, 0, stream, m, pix_parts, g, replay, healed);
    else if (use_bg)
        hipLaunchKernelGGL((nmi_covered_pix_kernel<false, false>), grid, block, 0, stream, m, pix_parts, g, replay, healed);
    else
        hipLaunchKernelGGL((nmi_covered_pix_kernel<true, false>), grid, block, 0, stream, m, pix_parts, g, replay, healed);
    return hipGetLastError();
}

}  // namespace nmi
