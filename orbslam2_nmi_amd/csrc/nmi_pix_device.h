// nmi_pix_device.h -- the pixel-range kernels' shared device code (nmi_pix_kernel.hip, nmi_masked_pix_kernel.hip,
// nmi_covered_pix_kernel.hip): the dealing of the pair's pieces, the hand-off blocks (PixHeader, unit layout, tagged mask
// granules), the owner's merged decode and its final trees.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nmi_grid_device.h"

namespace nmi {

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// One helper's block in memory.  The counters travel as 8,192 16-byte UNITS -- but only the units that hold a count: most of
// a natural pair's joint histogram is empty, and the launch's hand-offs together (20 MB at 81 candidates x 3 ranges) otherwise
// run at the rate the memory system takes write-through stores.  A unit is what ONE LANE OF THE OWNER'S DECODE needs at once:
// unit (wave, pass, half) of lane l = the four packed words k = 4 half .. 4 half + 3 that decode_phase's lane l of that
// wave reads in that pass (decode_row / decode_word, nmi_grid_device.h: row wave + 64 pass + 16 (l / 16), words i + 16 k of the row), so the owner never
// reshuffles anything.  Which units came is said by 64-bit masks, one per (wave, k = 2 pass + half), and the masks double as
// the flags: each travels as two 8-byte granules {half of the mask, launch tag}, stored after the drain and the barrier, so
// a wave of the owner that finds the tag in its 16 granules has its masks AND knows the units are in memory.
constexpr int kUnits = kWords / 4;             // 8192
constexpr int kUnitsPerLane = kUnits / kBlock;  // 8
constexpr int kGranules = kWaves * kUnitsPerLane * 2;  // 256 per helper
struct PixHeader {
    unsigned long long granule[kGranules];  // [(wave * 8 + k) * 2 + half]: {mask half, tag}
    uint32_t side_key[kSide];               // the helper's flat-region side counters (fold_flat_chunk), 0 = free
    uint32_t side_cnt[kSide];
    uint32_t pad[16];
};
static_assert(sizeof(PixHeader) == 2048 + 128 && sizeof(PixHeader) % 128 == 0, "whole lines");

constexpr size_t kPixBlockBytes = sizeof(PixHeader) + (size_t)kWords * sizeof(uint32_t);
constexpr int kAuxSc1 = 16;  // cache-policy bits of the raw buffer intrinsics: sc1 (write-through store / L1-bypassing load)
constexpr int kMaxRanges = 5;  // a wave's 64 lanes poll 16 granules of each of at most 4 helpers

constexpr unsigned long long kPixTimeoutTicks = 200000ull;  // 2 ms of the 100 MHz clock; a hand-off takes microseconds

// Which pixels a workgroup adds.  The pair is cut into PIECES of 64 chunks of 16 pixels (what one wavefront loads at once: 1.6
// rows of a 640-pixel-wide frame) and the pieces are DEALT to the candidate's workgroups rather than cut into P contiguous
// ranges: flat regions (render background, the warped frame's border) and busy ones cost different time per pixel and sit in
// different parts of the frame -- with contiguous thirds the range at the bottom of the benchmark's frames took 7.9 us against
// 6.2 for the middle one, up to 10.4, and a candidate is as slow as its slowest helper.  Dealing with period L = own + (P - 1) * hlp
// pieces: the owner takes the first `own` pieces of every period, helper h the `hlp` pieces from own + (h - 1) * hlp on; own / L
// is the owner's share (the host's choice, NMI_OPT_PIX_OWNER_BIAS).  A workgroup's i-th piece is piece
// (i / cnt) * L + off + i % cnt of the frame; wavefront w takes i = 16 * iteration + w: scalar arithmetic only.
struct Deal {
    int L, off, cnt;      // period, this workgroup's first piece in a period, its pieces per period
    uint32_t magic;       // ceil(2^32 / cnt): i / cnt = umulhi(i, magic) (exact far beyond the 2^14 pieces of a 2^24-pixel frame)
    int n;                // pieces of this workgroup in the whole frame
};
// The dealing pattern of a launch, made by the host (launch_pix): the kernel does no division.
struct DealArgs {
    int own, hlp;                    // pieces per period of the owner / of each helper
    uint32_t own_magic, hlp_magic;   // ceil(2^32 / own), ceil(2^32 / hlp) (unused when the count is 1)
    int periods, rest;               // pieces of the frame = periods * L + rest, rest < L
    uint32_t total_magic;            // ceil(2^32 / candidates) (0 for one candidate): block -> (range, candidate)
};
__device__ __forceinline__ Deal make_deal(const DealArgs &g, int P, int q)
{
    Deal d;
    d.L = g.own + (P - 1) * g.hlp;
    d.off = q == 0 ? 0 : g.own + (q - 1) * g.hlp;
    d.cnt = q == 0 ? g.own : g.hlp;
    d.magic = q == 0 ? g.own_magic : g.hlp_magic;
    d.n = g.periods * d.cnt + min(max(g.rest - d.off, 0), d.cnt);
    return d;
}

template <bool SHIFTED>
__device__ __forceinline__ void histogram_dealt(Lds &lds, const GridArgs &a, const uint8_t *__restrict__ render, const uint8_t *__restrict__ warped,
                                                int wave, int lane, const Deal &d)
{
    // chunk c = the j-th 16-byte chunk of row y: byte y * width + 16 j of the frame, ry * width + 16 j of the render -- rows need not
    // be whole aligned chunks (histogram_phase's ROWS form, nmi_kernels.hip; row_rem = width % 16 pixels per row are left for
    // add_row_tails below)
    const int nchunks = a.height * a.chunks_per_row, last = nchunks - 1, row_rem = a.width - (a.chunks_per_row << 4);
    auto ldw = [&](int c) {
        c = min(c, last);
        return *reinterpret_cast<const uint4 *>(warped + (((uint32_t)c << 4) + (uint32_t)__mul24((int)__umulhi((uint32_t)c, a.cpr_magic), row_rem)));
    };
    auto ldr = [&](int c) {  // NMI.cu:82: row y of the frame meets row H-1-y of a bottom-up render
        c = min(c, last);
        const int y = (int)__umulhi((uint32_t)c, a.cpr_magic);
        const int ry = a.flip ? a.height - 1 - y : y;
        return *reinterpret_cast<const uint4 *>(render + (((uint32_t)(__mul24(y, a.flip_row) + c + a.flip_base) << 4) + (uint32_t)__mul24(ry, row_rem)));
    };
    // chunk of this lane in the workgroup's iteration `it`; beyond the workgroup's pieces: some chunk >= nchunks (not added)
    auto chunk_of = [&](int it) {
        const int i = it * kWaves + wave;  // wavefront-uniform
        const int g = d.cnt > 1 ? (int)__umulhi((uint32_t)i, d.magic) : i;
        const int t = g * d.L + d.off + (i - g * d.cnt);
        return i < d.n ? (t << 6) + lane : 0x7FFFFFC0;
    };
    const int iters = (d.n + kWaves - 1) / kWaves;  // workgroup-uniform
    if (d.off == 0 && row_rem > 0) {
        // the owner also adds the last width % 16 pixels of every row
        const int x0 = a.chunks_per_row << 4, n = a.height * row_rem;
        for (int t = wave * 64 + lane; t < n; t += kBlock) {
            const int y = t / row_rem, x = x0 + t - y * row_rem;
            uint32_t d1 = render[(a.flip ? a.height - 1 - y : y) * a.width + x], d2 = warped[y * a.width + x];
            if (SHIFTED) {
                d1 >>= a.shift;
                d2 >>= a.shift;
            }
            (void)__hip_atomic_fetch_add(&lds.joint[joint_word(d1, d2)], joint_inc(d2), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
    }
    if (iters <= 0) return;
    const bool try_flat = !(a.phase_mask & 4);
    int resume = -1;
    int c = chunk_of(0);
    uint4 wa = ldw(c), ra = ldr(c), wb, rb;
    for (int it = 0; it < iters; it += 2) {
        const int cb = chunk_of(it + 1);
        wb = ldw(cb);
        rb = ldr(cb);
        if (__builtin_expect(flat_hint(ra, wa), 0)) {
            resume = it;
            break;
        }
        if (c < nchunks) add_chunk<true, SHIFTED, 2, false>(lds, 0, ra, wa, a.shift, false);
        c = chunk_of(it + 2);
        wa = ldw(c);
        ra = ldr(c);
        if (__builtin_expect(flat_hint(rb, wb), 0)) {
            resume = it + 1;
            break;
        }
        if (cb < nchunks) add_chunk<true, SHIFTED, 2, false>(lds, 0, rb, wb, a.shift, false);
    }
    if (resume >= 0) {
        // careful loop: same adds, flat chunks folded (fold_flat_chunk); one chunk of prefetch
        int cc = chunk_of(resume);
        uint4 wc = ldw(cc), rc = ldr(cc);
#pragma unroll 1
        for (int it = resume; it < iters; ++it) {
            const int cn = chunk_of(it + 1);
            const uint4 wn = ldw(cn), rn = ldr(cn);
            if (cc < nchunks) add_chunk<true, SHIFTED, 2, true>(lds, 0, rc, wc, a.shift, try_flat);
            wc = wn;
            rc = rn;
            cc = cn;
        }
    }
}

__device__ __forceinline__ int unit_offset(int wave, int kk, int lane) { return (int)sizeof(PixHeader) + ((wave * kUnitsPerLane + kk) * 64 + lane) * 16; }

// The dealing pattern of a launch (host): own : hlp pieces per period, the closest to owner_share among periods of at most 48
// pieces, and the magic numbers that spare the kernel every division.
inline DealArgs pix_dealing(const GridArgs &a, int pix_parts, double owner_share)
{
    int own = 1, hlp = 1;
    const double f = owner_share < 0.02 ? 0.02 : (owner_share > 0.98 ? 0.98 : owner_share);
    double best = 2.0;
    for (int b = 1; b <= 12; ++b) {
        int o = (int)(f / (1.0 - f) * (pix_parts - 1) * b + 0.5);
        o = o < 1 ? 1 : o;
        if (o + (pix_parts - 1) * b > 48) break;
        const double err = fabs((double)o / (o + (pix_parts - 1) * b) - f);
        constexpr double kCloser = 0.03;
        if (err < best - kCloser) best = err, own = o, hlp = b;  // a longer period has to be clearly closer: dealt in runs of 5 pieces
                                                                  // (8 rows) one helper was 16 % slower than the other on the benchmark's frames
    }
    auto magic = [](int d) { return d > 1 ? (uint32_t)((0x100000000ull + (uint32_t)d - 1) / (uint32_t)d) : 0u; };
    const int pieces = (a.height * a.chunks_per_row + 63) >> 6, L = own + (pix_parts - 1) * hlp;
    return DealArgs{own, hlp, magic(own), magic(hlp), pieces / L, pieces % L, magic(a.S_local * a.Wn)};
}

// What every pixel-range launch needs (host): 2 .. kMaxRanges ranges of a non-empty grid, frames of at least 32 pixels of width,
// the hand-off blocks, the packed counters (variant 3), the background rule on below 256 bins, the plain visiting order.
inline bool pix_launch_ok(const GridArgs &a, int pix_parts, bool use_bg)
{
    const long long total = (long long)a.S_local * a.Wn;
    if (pix_parts < 2 || pix_parts > kMaxRanges || total <= 0 || total * pix_parts > 0x7FFFFFFFll) return false;
    return !(a.width < 32 || !a.blocks || a.hist_variant != 3 || (a.shift != 0 && !use_bg) || a.order);
}

// The owner's decode: decode_phase (ComputeEntropyKernel + AddvectorParwiseMidKernel, NMI.cu:230-287) over its own packed
// counters PLUS the helpers' (acc: their units of this lane, already summed field by field), with two differences: counters
// are not cleared (the workgroup scores one candidate) and there are no wrap events to replay (nobody used returning atomics).
// TWIN: covered_decode_merged (nmi_covered_pix_kernel.hip) is a copy with per-candidate terms -- a fix here belongs there too.
template <bool ZERO0>
__device__ __forceinline__ void decode_merged(Lds &lds, const GridArgs &a, int wave, int lane, const u32x4 (&acc)[kUnitsPerLane])
{
    const bool side_any = lds.side_key[0][0] != 0u;
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
        if (__builtin_expect(side_any, 0)) {
            // side counters of flat regions (fold_flat_chunk): entries fill in order, a free one ends the list
            for (int e = 0; e < kSide; ++e) {
                const uint32_t key1 = __builtin_amdgcn_readfirstlane(lds.side_key[0][e]);
                if (key1 == 0u) break;
                const uint32_t sd1 = (key1 - 1u) >> 8, sd2 = (key1 - 1u) & 0xFFu;
                if (!in_decode_pass(sd1, wave, pass)) continue;  // not among this pass's 4 rows
                const uint32_t sword = joint_word(sd1, sd2);
                const uint32_t cnt = lds.side_cnt[0][e];
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    if (decode_word(d1, i, k) == sword) {
                        if (sd2 & 128u)
                            hi[k] += cnt;
                        else
                            lo[k] += cnt;
                    }
                }
            }
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
                if (lo[k] >= (uint32_t)kLdsTable) tl[k] = a.table[min(lo[k], (uint32_t)a.npix)];  // (a wrapped helper field can read high; the detector rejects the candidate)
                if (hi[k] >= (uint32_t)kLdsTable) th[k] = a.table[min(hi[k], (uint32_t)a.npix)];
            }
        }
        rsum = row_sum_16(rsum);
        if (!ZERO0) wave_total += rsum;
        const float x = row_tree_16(lane_tree_16(tl, th));
        if (i == 0) {
            lds.hist_render[d1] = rsum;
            lds.joint_row_sums[d1] = x;
        }
        if (a.dbg_joint) {
            uint32_t *row = a.dbg_joint + d1 * kBins;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int q = i + 16 * k;
                row[q] = lo[k];
                row[q + 128] = hi[k];
            }
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

// final_phase (nmi_kernels.hip: the three 256-element trees of AddVectorPairwiseKernel, NMI.cu:295-339, side by side in DPP rows
// 0..2, then the score) with one difference: the marginal counts' terms come from the LDS copy of the table where the count is
// below its 4096 entries (most of a 640x480 frame's 256 marginal bins are) and from memory only above -- the owner scores ONE
// candidate, so the memory round trip of the lookups is on every launch's critical path instead of hidden behind the next
// candidate's pixels.  Same values (the LDS table is a copy), same order.
__device__ __forceinline__ void final_phase_owner(Lds &lds, const GridArgs &a, int lane, int p, int w, int s, unsigned long long &prev_key)
{
    const int i = lane & 15, r = lane >> 4;
    float lo[8], hi[8];
    const uint32_t *h = r == 0 ? lds.hist_render : lds.hist_warped;
    uint32_t cl[8], ch[8], cmax = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        cl[k] = r < 2 ? h[i + 16 * k] : 0u;
        ch[k] = r < 2 ? h[i + 16 * k + 128] : 0u;
        cmax = max(cmax, max(cl[k], ch[k]));
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        lo[k] = lds.table[cl[k] & (kLdsTable - 1)];
        hi[k] = lds.table[ch[k] & (kLdsTable - 1)];
    }
    if (cmax >= (uint32_t)kLdsTable) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (cl[k] >= (uint32_t)kLdsTable) lo[k] = a.table[cl[k]];
            if (ch[k] >= (uint32_t)kLdsTable) hi[k] = a.table[ch[k]];
        }
    }
    if ((w == 0 || s == 0) && a.plan) {  // the search as its own content probe (final_phase)
        uint32_t m = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) m |= (cl[k] != 0u ? 1u << k : 0u) | (ch[k] != 0u ? 0x100u << k : 0u);
        if (lane < 32 && m) __hip_atomic_fetch_or(const_cast<uint32_t *>(&a.plan->seen[lane]), m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
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
    if (a.dbg_h1 && lane < 64) {
        for (int t = lane; t < kBins; t += 64) {
            a.dbg_h1[t] = lds.hist_render[t];
            if (a.dbg_h2) a.dbg_h2[t] = lds.hist_warped[t];
        }
    }
    if (lane == 0) commit_score(a, p, w, s, a1, a2, a3, prev_key);
}

}  // namespace

}  // namespace nmi
