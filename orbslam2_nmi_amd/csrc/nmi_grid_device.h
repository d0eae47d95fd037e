// nmi_grid_device.h -- nmi_grid_kernel's device functions (nmi_grid_kernel.h), shared by every scoring kernel that keeps
// a whole packed joint histogram per workgroup: the LDS layout, the seams of a candidate (clear_lds, retire_candidate), the chunk /
// pixel adders, histogram_phase, decode_phase, final_phase, finish_search and exact_candidate.  Everything is in an unnamed
// namespace: each translation unit gets its own copy, inlined into its own kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nmi_kernels.h"
#include "nmi_device.h"

namespace nmi {

namespace {

constexpr int kBlock = NMI_BLOCK_THREADS;  // 1024 lanes = 16 wavefronts, one workgroup per CU (LDS-limited)
constexpr int kWaves = kBlock / 64;
constexpr int kBins = 256;
constexpr int kWords = kBins * kBins / 2;  // two 16-bit counters per LDS word
constexpr int kRowStride = 129;            // LDS words from one joint row to the next: 128 counter words + 1 unused (see joint_word)
constexpr int kJointWords = kBins * kRowStride;  // the LDS array: the kWords counter words and the 256 gap words (always zero)
constexpr int kOvfCap = 1024;              // >= 2 * floor(2^24 / 65536) + 1 wrap events per candidate
constexpr int kRowsPerWave = kBins / kWaves;
constexpr int kLdsTable = 4096;            // per-count entropy terms kept in LDS for counts below this
constexpr int kSide = 8;                   // side counters for bins fed by flat image regions (see fold_flat_chunk)

// LDS word of joint bin (d1 = render intensity, d2 = warped-frame intensity):
//   word = d1 * kRowStride + (d2 & 127), low half for d2 < 128, high half for d2 >= 128.
// Each word thus holds the pair (d2, d2 + 128) -- the two operands of the first tree step a[t] += a[t+128]
// (NMI.cu:276-284) -- and a lane that owns the words i, i+16, ..., i+112 of a row owns all operands of the steps
// n = 128, 64, 32, 16 (decode_phase).  A row is 129 words long, not 128: row d1 occupies [129 d1, 129 d1 + 127], the word
// after it is never touched, nothing wraps inside a row -- and the LDS bank of a bin is (d1 + d2) & 31.  With 128 it was
// d2 & 31 alone, and the zero border of a warped frame (3-4.5 % of the pixels of a search's warps) put every lane that
// met it on bank 0, in a different word per render intensity.

struct Lds {
    uint32_t joint[kJointWords];  // 129 KiB
    uint32_t hist_render[kBins];
    uint32_t hist_warped[kBins];
    float joint_row_sums[kBins];  // d_JointEntropyShort, kernel.cu:60,90
    uint32_t ovf[2][kOvfCap];     // wrap events: (word << 1) | field; double-buffered by candidate parity
    uint32_t ovf_n[2];
    uint32_t total[2];            // sum of all decoded counters of the candidate (wrap detector), by parity
    uint32_t side_key[2][kSide];  // flat-region side counters: the bin ((d1 << 8) | d2) + 1, 0 = free; by candidate parity
    uint32_t side_cnt[2][kSide];  // their 32-bit counts (added to the decoded counters in decode_phase)
    float table[kLdsTable];       // table[c] for c < kLdsTable (16 KiB); larger counts read the global table
    uint32_t fallback;            // pipelined kernel: a candidate wrapped, finish sequentially on the exact path
    uint32_t redo_n;
    uint32_t redo[4];             // ordinals (within this workgroup) of candidates to score again exactly
};

// Candidate visited by workgroup `b` in its round `r`.  Workgroups are dealt to the 8 XCDs round-robin (b and b + 8
// share an XCD and its L2), so the 32 workgroups of an XCD take 32 CONSECUTIVE ordinals of the visiting order, and the
// host lays the order out in tiles of (few warps) x (few renders): an XCD's round then touches ~12 images (~3.6 MB at
// 640x480, inside its 4 MiB L2) instead of ~29.  nmi_grid_kernel's own plain searches read an order that also keeps one warp per
// workgroup over its rounds (build_search_order, nmi_search_plan.h: 13-14 images per XCD and round for 27 x 27), so that the frame
// marginal is formed once per workgroup.  Placement is a speed matter only; any order gives the same results.
// (slot_in_round: nmi_device.h)
__device__ __forceinline__ int candidate_at(const GridArgs &a, int ordinal) { return a.order ? a.order[ordinal] : ordinal; }

// ---- the seams of the one-workgroup-per-candidate kernels (nmi_grid_kernel keeps its own text: profiles/grid_templates) ----
// The small state beside the joint words to zero: the frame marginal, both parities' event counts and totals, the side counters
// (kernels that never fold a flat chunk never set those, but decode_phase reads them).  A function of its own: written out inside
// clear_lds, the same statements changed the machine code of 25 kernels instead of 12 (profiles/grid_templates/isa_vs_parent.txt).
__device__ __forceinline__ void clear_candidate_state(Lds &lds, int tid)
{
    if (tid < kBins) lds.hist_warped[tid] = 0;
    if (tid < 2) lds.ovf_n[tid] = lds.total[tid] = 0;
    if (tid < 2 * kSide) (&lds.side_key[0][0])[tid] = (&lds.side_cnt[0][0])[tid] = 0;
}
// Every counter of the workgroup to zero, before its first candidate.
__device__ __forceinline__ void clear_lds(Lds &lds, int tid)
{
    uint4 *j4 = reinterpret_cast<uint4 *>(lds.joint);
    const uint4 z = {0, 0, 0, 0};
    for (int i = tid; i < kJointWords / 4; i += kBlock) j4[i] = z;
    clear_candidate_state(lds, tid);
}
// Wavefront 0 after it has scored the candidate of parity `par`, while the others add the next one's pixels.
__device__ __forceinline__ void retire_candidate(Lds &lds, int par, int lane)
{
    for (int t = lane; t < kBins; t += 64) lds.hist_warped[t] = 0;
    if (lane == 0) {
        lds.ovf_n[par] = 0;      // consumed by this candidate's decode; next used two candidates on
        lds.total[par ^ 1] = 0;  // read by everyone right after the previous B2; next candidate adds to it
    }
}

// ---- histogram phase -------------------------------------------------------------------------------
// One pixel -> one LDS atomic on the packed joint histogram (the reference does three atomics per
// pixel, NMI.cu:46-48; the marginals are recovered as row / column sums of the joint).
// Each 16-bit field is only ever incremented by one, by an add that returns the old word, so every
// wrap of a field is seen by exactly one lane: a low-field wrap carries into the high field (the
// high field then counts d2>=128 hits plus low wraps), a high-field wrap is seen either by a high
// add (old high == 0xFFFF) or by the carrying low add (old word == 0xFFFFFFFF).  Events are rare
// (at most about 2 * W*H / 65536 per candidate) and are replayed when the counters are decoded.
__device__ __forceinline__ uint32_t joint_word(uint32_t d1, uint32_t d2) { return d1 * (uint32_t)kRowStride + (d2 & 127u); }
__device__ __forceinline__ uint32_t joint_inc(uint32_t d2) { return (d2 & 128u) ? 0x10000u : 1u; }

__device__ __forceinline__ void record_wrap(Lds &lds, int par, uint32_t word, uint32_t val, uint32_t old)
{
    uint32_t k = __hip_atomic_fetch_add(&lds.ovf_n[par], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (k < kOvfCap) lds.ovf[par][k] = (word << 1) | (val >> 16);
    if (val == 1u && old == 0xFFFFFFFFu) {
        k = __hip_atomic_fetch_add(&lds.ovf_n[par], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (k < kOvfCap) lds.ovf[par][k] = (word << 1) | 1u;
    }
}

template <bool BG, bool SHIFTED>
__device__ __forceinline__ void add_pixel(Lds &lds, int par, uint32_t d1, uint32_t d2, int shift)
{
    if (!BG && (d1 == 0 || d2 == 0)) return;  // NMI.cu:85
    if (SHIFTED) {
        d1 >>= shift;
        d2 >>= shift;
    }
    const uint32_t word = joint_word(d1, d2), val = joint_inc(d2);
    const uint32_t old = __hip_atomic_fetch_add(&lds.joint[word], val, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    const uint32_t field = val * 0xFFFFu;
    if (__builtin_expect((old & field) == field, 0)) record_wrap(lds, par, word, val, old);
}

// Flat chunks.  When, for every active lane of the wavefront, all 16 pixels of the lane carry the same (render, frame)
// pair -- render background over saturated sky or over the frame border, clipped regions -- the plain path would queue
// 64 lanes on one LDS address 16 times over (2 cycles per lane each time: ~12x the cost of a textured chunk).  Folded,
// the 16 updates of a lane become one weighted add, and if the whole wavefront agrees on the pair, one add by one lane
// into a 32-bit side counter (kSide per candidate, replayed in decode_phase): a large flat region then neither
// serialises the LDS nor wraps a 16-bit field, so such frames stay on the one-pass optimistic path.
// Returns false (nothing done) when some active lane is not flat.
__device__ __forceinline__ bool side_add(Lds &lds, int par, uint32_t d1, uint32_t d2, uint32_t weight)
{
    const uint32_t key1 = ((d1 << 8) | d2) + 1u;
    for (int e = 0; e < kSide; ++e) {
        const uint32_t old = atomicCAS(&lds.side_key[par][e], 0u, key1);
        if (old == 0u || old == key1) {
            atomicAdd(&lds.side_cnt[par][e], weight);
            return true;
        }
    }
    return false;
}

template <bool BG, bool SHIFTED, int HIST>
__device__ __forceinline__ bool fold_flat_chunk(Lds &lds, int par, const uint32_t (&r)[4], const uint32_t (&w)[4], int shift)
{
    const uint32_t rb = r[0] & 0xFFu, wb = w[0] & 0xFFu;
    const bool flat = r[0] == r[1] && r[1] == r[2] && r[2] == r[3] && w[0] == w[1] && w[1] == w[2] && w[2] == w[3] &&
                      r[0] == rb * 0x01010101u && w[0] == wb * 0x01010101u;
    if (!__all(flat)) return false;
    uint32_t d1 = rb, d2 = wb;
    const bool skip = !BG && (d1 == 0 || d2 == 0);  // NMI.cu:85
    if (SHIFTED) {
        d1 >>= shift;
        d2 >>= shift;
    }
    const uint32_t key = (d1 << 8) | d2;
    const uint32_t key0 = __builtin_amdgcn_readfirstlane(key);
    const bool skip0 = __builtin_amdgcn_readfirstlane((uint32_t)skip) != 0;
    const uint32_t word = joint_word(d1, d2), high = d2 >> 7;
    uint32_t weight = 16;
    bool issue = !skip;
    if (__all(key == key0 && skip == skip0)) {  // one lane speaks for the wavefront
        const unsigned long long active = __ballot(1);
        weight = 16u * (uint32_t)__popcll(active);
        issue = issue && (__lane_id() == (uint32_t)__ffsll((long long)active) - 1u);
        if (issue && side_add(lds, par, d1, d2, weight)) issue = false;
    }
    if (issue) {
        const uint32_t inc = high ? weight << 16 : weight;
        if (HIST == 2) {
            (void)__hip_atomic_fetch_add(&lds.joint[word], inc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        } else {
            const uint32_t old = __hip_atomic_fetch_add(&lds.joint[word], inc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            const uint32_t field_old = high ? old >> 16 : old & 0xFFFFu;
            if (field_old + weight > 0xFFFFu) record_wrap(lds, par, word, high ? 0x10000u : 1u, high ? old : (old | 0xFFFFu));
        }
    }
    return true;
}

// 16 pixels of one lane.  HIST selects how wraps of the 16-bit counters are handled:
//   0  returning atomic + test per pixel (serialises on the LDS round trip; kept as the ablation baseline)
//   1  16 returning atomics in flight, one combined wrap test per 16 pixels, flat chunks folded (the exact path)
//   2  non-returning atomics, no test: exact only when no bin can exceed 65535 (first try of the
//      optimistic scheme HIST = 3, see nmi_grid_kernel)
template <bool BG, bool SHIFTED, int HIST, bool FOLD>
__device__ __forceinline__ void add_chunk(Lds &lds, int par, const uint4 &rv, const uint4 &wv, int shift, bool try_flat)
{
    const uint32_t r[4] = {rv.x, rv.y, rv.z, rv.w};
    const uint32_t w[4] = {wv.x, wv.y, wv.z, wv.w};
    if (HIST == 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                add_pixel<BG, SHIFTED>(lds, par, (r[q] >> (8 * j)) & 0xFFu, (w[q] >> (8 * j)) & 0xFFu, shift);
        return;
    }
    // Flat chunks (render background over saturated sky or frame border, ...) are folded, see fold_flat_chunk; only the
    // careful loop of histogram_phase asks for it.
    if (FOLD && HIST != 0 && try_flat) {
        if (__builtin_expect(flat_hint(rv, wv), 0)) {
            if (fold_flat_chunk<BG, SHIFTED, HIST>(lds, par, r, w, shift)) return;
        }
    }
    if (HIST == 2 && BG && !SHIFTED) {
        // The hot case, written so that each pixel costs 5 VALU + 1 DS: byte address = d1 * 516 + (d2 & 127) * 4 from one
        // byte-select 24-bit multiply of the render dword (the row's byte address), one bit-field extract of the frame dword
        // and one shift-add; increment 1 + 0xFFFF * bit7(d2) from a second extract and a 24-bit multiply-add.  hipcc derives
        // more from the plain C expressions (a separate mask for the render byte; mask + compare + select for the
        // increment), so the SDWA multiply and the multiply-add are spelled out.
        char *const base = reinterpret_cast<char *>(lds.joint);
        const uint32_t row_bytes = kRowStride * 4, k_ffff = 0xFFFFu;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                uint32_t a1, c, addr, hi, val;
                if (j == 0)
                    asm("v_mul_u32_u24_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_0 src1_sel:DWORD" : "=v"(a1) : "v"(r[q]), "s"(row_bytes));
                else if (j == 1)
                    asm("v_mul_u32_u24_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_1 src1_sel:DWORD" : "=v"(a1) : "v"(r[q]), "s"(row_bytes));
                else if (j == 2)
                    asm("v_mul_u32_u24_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_2 src1_sel:DWORD" : "=v"(a1) : "v"(r[q]), "s"(row_bytes));
                else
                    asm("v_mul_u32_u24_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_3 src1_sel:DWORD" : "=v"(a1) : "v"(r[q]), "s"(row_bytes));
                c = __builtin_amdgcn_ubfe(w[q], 8 * j, 7);
                asm("v_lshl_add_u32 %0, %1, 2, %2" : "=v"(addr) : "v"(c), "v"(a1));
                hi = __builtin_amdgcn_ubfe(w[q], 8 * j + 7, 1);
                asm("v_mad_u32_u24 %0, %1, %2, 1" : "=v"(val) : "v"(hi), "s"(k_ffff));
                (void)__hip_atomic_fetch_add(reinterpret_cast<uint32_t *>(base + addr), val, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
        }
        return;
    }
    uint32_t old[16];
    uint32_t any = 0;  // max over pixels of (old | ~field): 0xFFFFFFFF iff some counter wrapped
#pragma unroll
    for (int q = 0; q < 4; ++q) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            uint32_t d1 = (r[q] >> (8 * j)) & 0xFFu, d2 = (w[q] >> (8 * j)) & 0xFFu;
            const bool skip = !BG && (d1 == 0 || d2 == 0);  // NMI.cu:85
            if (SHIFTED) {
                d1 >>= shift;
                d2 >>= shift;
            }
            const uint32_t word = joint_word(d1, d2), val = joint_inc(d2);
            if (HIST == 2) {
                if (!skip) (void)__hip_atomic_fetch_add(&lds.joint[word], val, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            } else {
                old[q * 4 + j] = 0;
                if (!skip)
                    old[q * 4 + j] = __hip_atomic_fetch_add(&lds.joint[word], val, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
        }
    }
    if (HIST == 1) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                uint32_t d2 = (w[q] >> (8 * j)) & 0xFFu;
                if (SHIFTED) d2 >>= shift;
                const uint32_t notfield = (d2 & 128u) ? 0x0000FFFFu : 0xFFFF0000u;
                const uint32_t t = old[q * 4 + j] | notfield;
                any = t > any ? t : any;
            }
        if (__builtin_expect(any == 0xFFFFFFFFu, 0)) {
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    uint32_t d1 = (r[q] >> (8 * j)) & 0xFFu, d2 = (w[q] >> (8 * j)) & 0xFFu;
                    const bool skip = !BG && (d1 == 0 || d2 == 0);
                    if (SHIFTED) {
                        d1 >>= shift;
                        d2 >>= shift;
                    }
                    const uint32_t val = joint_inc(d2), field = val * 0xFFFFu;
                    if (!skip && (old[q * 4 + j] & field) == field) record_wrap(lds, par, joint_word(d1, d2), val, old[q * 4 + j]);
                }
        }
    }
}

// Histogram phase for one candidate: histogram256Kernel's pixel loop, NMI.cu:79-87.
// NT lanes (tid = 0..NT-1) share the pixels of the candidate -- on the 16-byte path the 16-pixel chunks [c_first, c_end)
// of it (the whole pair: 0, npix / 16; nmi_pix_kernel.hip gives each of a candidate's workgroups a range of its own).
// ROWS (GridRows, nmi_kernels_rows.hip, only): rows that are not whole aligned chunks -- width % 16 != 0 (KITTI's 1241 x 376), or stacks
// that are not 16-byte aligned.  Chunk c = (row y, j-th chunk of the row) starts at byte y * width + 16 j of the frame and at
// ry * width + 16 j of the render (unaligned 16-byte loads); the width % 16 pixels left at the end of every row are added one
// by one after the loop.  c_end is then height * (width / 16).  (Through the byte path below such frames took 4.1x the time per
// pixel: profiles/r04_a/odd_width_time.txt.)
//
// SLABS (nmi_grid_kernel's hot loop only): shares of the chunks by wavefront age.  A SIMD serves its oldest wavefront first, so
// with equal shares (chunk = c_first + tid + it * NT) wavefronts 0-3 were done at 12.4 us of a 21.7 us phase, 4-7 at 14.2, 8-11 at
// 19.1, and the LDS unit spent the last 9 us fed by 12, 8, 4 wavefronts (profiles/r04_c/grid_stamps_27x27_clock.txt).  Instead
// [c_first, c_end) is cut into 16 contiguous slabs, wavefront v walks slab v 64 chunks at a time (chunk = base[v] + it * 64 + lane),
// and the slabs' lengths follow the rates the wavefronts really run at, so that all 16 end together.  Slab v is
// [n * cum[v] >> 16, n * cum[v + 1] >> 16) of the n chunks: one scalar multiply and shift each, the end of one slab is the base
// of the next, every chunk is covered once at any n.  Two rows of cumulative Q16 shares: a workgroup's first candidate, and its
// later ones, where wavefront 0 scores the previous candidate (final_phase, ~2.5 us) before it adds its first pixel.
// Calibrated on MI355X with tools/grid_stamps.py (profiles/NOTES.md, "Pixel shares by wavefront age"); a matter of speed only.
#ifndef NMI_SLAB_SHARES_QUALIFIER
#define NMI_SLAB_SHARES_QUALIFIER __constant__ const
#endif
NMI_SLAB_SHARES_QUALIFIER uint32_t slab_cum[2][kWaves + 1] = {
    {0, 7048, 14096, 21145, 28193, 34369, 40546, 46722, 52899, 55010, 57120, 59231, 61342, 62390, 63439, 64487, 65536},
    {0, 5934, 12896, 19858, 26820, 33147, 39384, 45621, 51859, 54448, 56633, 58818, 61003, 62222, 63327, 64431, 65536},
};

template <bool BG, bool SHIFTED, int HIST, int NT, bool FOLD = true, bool ROWS = false, bool SLABS = false>
__device__ __forceinline__ void histogram_phase(Lds &lds, int par, const GridArgs &a, const uint8_t *__restrict__ render,
                                                const uint8_t *__restrict__ warped, int tid, int c_first, int c_end, bool later = false)
{
    static_assert(!SLABS || NT == kBlock, "slabs are per wavefront of a whole workgroup");
    if (ROWS || a.vec_ok) {
        // 16 pixels per lane per step: one 16-byte load from each image (1 KiB per wavefront instruction),
        // the next step's loads issued before this step's atomics.
        const int nchunks = c_end;
        // 32-bit unsigned byte offsets from the (scalar) image bases: one shift per load instead of 64-bit pointer math
        const int row_rem = ROWS ? a.width - (a.chunks_per_row << 4) : 0;  // pixels of a row beyond its whole chunks
        auto ldw = [&](int c) {
            if (ROWS) return *reinterpret_cast<const uint4 *>(warped + (((uint32_t)c << 4) + (uint32_t)__mul24((int)__umulhi((uint32_t)c, a.cpr_magic), row_rem)));
            return *reinterpret_cast<const uint4 *>(warped + ((uint32_t)c << 4));
        };
        // NMI.cu:82: row y of the frame meets row H-1-y of a bottom-up render.  Branch-free for both orientations:
        // render chunk = c + flip_base + y * flip_row with y = c / chunks_per_row (multiply-high by the magic).
        auto ldr = [&](int c) {
            const int y = (int)__umulhi((uint32_t)c, a.cpr_magic);
            if (ROWS) {
                const int ry = a.flip ? a.height - 1 - y : y;
                return *reinterpret_cast<const uint4 *>(render + (((uint32_t)(__mul24(y, a.flip_row) + c + a.flip_base) << 4) + (uint32_t)__mul24(ry, row_rem)));
            }
            return *reinterpret_cast<const uint4 *>(render + ((uint32_t)(__mul24(y, a.flip_row) + c + a.flip_base) << 4));
        };
        // Fast loop.  Software pipeline with two named register sets: the loads of the chunk after next are in flight
        // while the current chunk's 16 atomics issue (a third set measured no faster and costs 8 VGPRs).  Loads are
        // unconditional (index clamped to the last chunk, a valid address) so the code is straight-line and the
        // compiler can wait on exact load counts; only the atomics are predicated on the chunk being in range.
        // The only trace of the flat-region handling in here is flat_hint + a branch that is never taken on textured
        // content: on a hit the wavefront leaves for the careful loop below and stays there for the rest of this
        // candidate (everything the fold needs inside this loop cost 5-11 % of the whole kernel).
        constexpr bool kHint = FOLD && HIST != 0;
        const bool try_flat = kHint && !(a.phase_mask & 4);  // bit 2: ablation switch (careful loop entered, nothing folded)
        // This lane walks the chunks first, first + kStep, ... below `stop`; prefetch indices are clamped to `last`.
        constexpr int kStep = SLABS ? 64 : NT;
        int base = c_first, stop = nchunks, first = c_first + tid;
        if (SLABS) {  // this wavefront's slab [base, stop): wavefront-uniform (scalar)
            const uint32_t v = __builtin_amdgcn_readfirstlane((uint32_t)tid >> 6), n = (uint32_t)(nchunks - c_first);
            const uint32_t *cum = slab_cum[later ? 1 : 0];
            base = c_first + (int)(((unsigned long long)n * cum[v]) >> 16);
            stop = c_first + (int)(((unsigned long long)n * cum[v + 1]) >> 16);
            first = base + (tid & 63);
        }
        const int last = SLABS ? max(stop, c_first + 1) - 1 : nchunks - 1;  // (an empty slab: still an address inside the images)
        const int iters = (stop - base + kStep - 1) / kStep;  // wavefront-uniform
        int resume = (HIST == 1 && kHint) ? first : -1;  // the exact path is cold anyway: careful from the start
        if (resume < 0) {
            int ch = first;
            int c0 = min(ch, last);
            uint4 wa = ldw(c0), ra = ldr(c0), wb, rb;
            for (int it = 0; it < iters; it += 2) {
                const int c1 = min(ch + kStep, last);
                wb = ldw(c1);
                rb = ldr(c1);
                if (kHint && __builtin_expect(flat_hint(ra, wa), 0)) {
                    resume = ch;
                    break;
                }
                if (ch < stop) add_chunk<BG, SHIFTED, HIST, false>(lds, par, ra, wa, a.shift, false);
                const int c2 = min(ch + 2 * kStep, last);
                wa = ldw(c2);
                ra = ldr(c2);
                if (kHint && __builtin_expect(flat_hint(rb, wb), 0)) {
                    resume = ch + kStep;
                    break;
                }
                if (ch + kStep < stop) add_chunk<BG, SHIFTED, HIST, false>(lds, par, rb, wb, a.shift, false);
                ch += 2 * kStep;
            }
        }
        if (resume >= 0) {
            // Careful loop: same adds, flat chunks folded; one chunk of prefetch.
            int c = min(resume, last);
            uint4 wc = ldw(c), rc = ldr(c);
#pragma unroll 1
            for (int ch = resume; ch < stop; ch += kStep) {
                const int cn = min(ch + kStep, last);
                const uint4 wn = ldw(cn), rn = ldr(cn);
                add_chunk<BG, SHIFTED, HIST, true>(lds, par, rc, wc, a.shift, try_flat);
                wc = wn;
                rc = rn;
            }
        }
        if (ROWS && row_rem > 0) {
            // the last width % 16 pixels of every row
            const int x0 = a.chunks_per_row << 4, n = a.height * row_rem;
            for (int t = tid; t < n; t += NT) {
                const int y = t / row_rem, x = x0 + t - y * row_rem;
                const int ry = a.flip ? (a.height - 1 - y) : y;
                uint32_t d1 = render[ry * a.width + x], d2 = warped[y * a.width + x];
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
    } else {
        // Any width / alignment: byte loads, position arithmetic as written in NMI.cu:79-83.
        for (int pos = tid; pos < a.npix; pos += NT) {
            const int y = pos / a.width;
            const int x = pos - y * a.width;
            const int ry = a.flip ? (a.height - 1 - y) : y;
            if (HIST == 2) {
                uint32_t d1 = render[ry * a.width + x], d2 = warped[pos];
                if (BG || (d1 != 0 && d2 != 0)) {
                    if (SHIFTED) {
                        d1 >>= a.shift;
                        d2 >>= a.shift;
                    }
                    (void)__hip_atomic_fetch_add(&lds.joint[joint_word(d1, d2)], joint_inc(d2), __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_WORKGROUP);
                }
            } else {
                add_pixel<BG, SHIFTED>(lds, par, render[ry * a.width + x], warped[pos], a.shift);
            }
        }
    }
}

__device__ __forceinline__ float term(const float *__restrict__ table, uint32_t c)
{
    // ComputeEntropyKernel, NMI.cu:242-263; table[c] = (c/len) * log2f(c/len), table[0] = 0.
    return c ? table[c] : 0.0f;
}
// Same value, served from the LDS copy of the table for the (overwhelmingly common) small counts.
__device__ __forceinline__ float term_lds(const Lds &lds, const float *__restrict__ table, uint32_t c)
{
    float t = lds.table[c < (uint32_t)kLdsTable ? c : 0u];
    if (__builtin_expect(c >= (uint32_t)kLdsTable, 0)) t = table[c];
    return t;
}

// Who decodes what: wavefront `wave` takes the 4 joint rows wave + 64 pass + 16 r of its pass `pass`, one per 16-lane DPP row
// r, and lane i of a DPP row the words i + 16 k (k = 0..7) of its row.  Every kernel that reads packed counters in decode
// order (decode_phase, the pixel-range hand-off units, the masked and covered forms, the ablation drain) goes through these.
static_assert(kWaves == 16 && (kWaves * kRowStride) % 32 == 16, "rows kWaves apart must fall on opposite halves of the 32 banks");
__device__ __forceinline__ int decode_row(int wave, int pass, int r) { return wave + 4 * kWaves * pass + kWaves * r; }
__device__ __forceinline__ bool in_decode_pass(uint32_t d1, int wave, int pass)
{
    return (d1 % (uint32_t)kWaves) == (uint32_t)wave && (d1 / (uint32_t)(4 * kWaves)) == (uint32_t)pass;
}
__device__ __forceinline__ uint32_t decode_word(int d1, int i, int k) { return (uint32_t)(d1 * kRowStride + i + 16 * k); }

// Replays the wrap events of one LDS word onto its two decoded counters.
__device__ __forceinline__ void apply_wraps(const Lds &lds, int par, uint32_t novf, uint32_t word, uint32_t &lo,
                                            uint32_t &hi)
{
    for (uint32_t e = 0; e < novf; ++e) {
        const uint32_t ev = lds.ovf[par][e];
        if ((ev >> 1) == word) {
            if (ev & 1u) {
                hi += 65536u;
            } else {
                lo += 65536u;
                hi -= 1u;  // the carry that the low wrap pushed into the high field
            }
        }
    }
}

// ---- decode phase: counters -> per-bin terms -> row trees (ComputeEntropyKernel + AddvectorParwiseMidKernel) ----
// A wavefront takes 4 joint rows per pass, one per 16-lane DPP row.  Lane i of a row owns the bins
// d2 = i + 16*j (j = 0..15): words i + 16*k (k = 0..7) hold the pairs (d2, d2 + 128).  Every tree step
// n >= 16 of NMI.cu:276-284 then pairs two values of the same lane and the steps n = 8..1 are DPP
// shifts inside the 16-lane row: no LDS traffic besides reading (and clearing) the counters.
// The rows of a pass are 16 apart (decode_row): 16 rows of 129 words shift the bank by 16, so the two rows of a 32-lane LDS
// access group hit disjoint halves of the banks, and a lane's eight words are constant offsets 16 k from one base.
// ZERO0 (background rule off, NMI.cu:85: a pixel counts only if both intensities are non-zero): the histogram phase
// has counted every pixel -- the skipped ones are exactly row 0 and column 0 of the joint histogram, which are cleared
// here, after they have entered the wrap detector's total.
// KEPT (nmi_grid_kernel's later candidates on one warp, every pixel counted): the frame marginal -- the column sums -- is the plain
// histogram of the warp image, the same for every render it meets; the workgroup formed it and its entropy sum on an earlier
// candidate (final_phase), so this form carries no column sums and ends without the 16 atomics per lane into hist_warped.
template <bool ZERO0 = false, bool KEPT = false>
__device__ __forceinline__ void decode_phase(Lds &lds, int par, const GridArgs &a, int wave, int lane)
{
    const uint32_t novf = lds.ovf_n[par] < (uint32_t)kOvfCap ? lds.ovf_n[par] : (uint32_t)kOvfCap;
    const bool side_any = lds.side_key[par][0] != 0u;
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
        if (__builtin_expect(side_any, 0)) {
            // side counters of flat regions (fold_flat_chunk): entries fill in order, a free one ends the list
            for (int e = 0; e < kSide; ++e) {
                const uint32_t key1 = __builtin_amdgcn_readfirstlane(lds.side_key[par][e]);
                if (key1 == 0u) break;
                const uint32_t sd1 = (key1 - 1u) >> 8, sd2 = (key1 - 1u) & 0xFFu;
                if (!in_decode_pass(sd1, wave, pass)) continue;  // not among this pass's 4 rows
                const uint32_t sword = joint_word(sd1, sd2);
                const uint32_t cnt = lds.side_cnt[par][e];
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    if (a0 + 16 * k == sword) {
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
            if (!KEPT) {
                col_lo[k] += lo[k];
                col_hi[k] += hi[k];
            }
            rsum += lo[k] + hi[k];
            cmax = max(cmax, max(lo[k], hi[k]));
            // straight-line LDS lookups; counts beyond the LDS table are patched below (one branch per pass)
            tl[k] = lds.table[lo[k] & (kLdsTable - 1)];
            th[k] = lds.table[hi[k] & (kLdsTable - 1)];
        }
        if (__builtin_expect(cmax >= (uint32_t)kLdsTable, 0)) {
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                if (lo[k] >= (uint32_t)kLdsTable) tl[k] = a.table[lo[k]];
                if (hi[k] >= (uint32_t)kLdsTable) th[k] = a.table[hi[k]];
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
    if (!KEPT) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int q = i + 16 * k;
            atomicAdd(&lds.hist_warped[q], col_lo[k]);
            atomicAdd(&lds.hist_warped[q + 128], col_hi[k]);
        }
    }
    if (i == 0) atomicAdd(&lds.total[par], wave_total);
}

// Final stage, one wavefront: the three 256-element trees of AddVectorPairwiseKernel (NMI.cu:295-339) run
// side by side in DPP rows 0 (render marginal), 1 (frame marginal), 2 (joint row sums); then the score.
// `kept` (nmi_grid_kernel only, see decode_phase<.., true>): hist_warped was not formed for this candidate; row 1 idles and the
// frame marginal's sum is *frame_sum, where the call that formed it for this warp left it (any call with frame_sum and !kept).
__device__ __forceinline__ void final_phase(Lds &lds, const GridArgs &a, int lane, int p, int w, int s,
                                            unsigned long long &prev_key, bool kept = false, float *frame_sum = nullptr)
{
    const int i = lane & 15, r = lane >> 4;
    float lo[8], hi[8];
    // All 16 table lookups of a lane are issued back to back and unconditionally (table[0] = 0; rows 2, 3 fetch
    // table[0] and discard it): one memory round trip (1.0 us) instead of one per conditional lookup (2.5 us).  The
    // other wavefronts are already adding the next candidate's pixels and wait for this one at the next barrier.
    const uint32_t *h = r == 0 ? lds.hist_render : lds.hist_warped;
    uint32_t cl[8], ch[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        cl[k] = r < (kept ? 1 : 2) ? h[i + 16 * k] : 0u;
        ch[k] = r < (kept ? 1 : 2) ? h[i + 16 * k + 128] : 0u;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        lo[k] = a.table[cl[k]];
        hi[k] = a.table[ch[k]];
    }
    if ((w == 0 || s == 0) && a.plan) {
        // The search as its own content probe (NMI_OPT_CONTENT_PATH): which bins do the two marginals hold?  16 flags per lane
        // of DPP rows 0 and 1, ORed into the plan's masks (LevelPlan::seen) while the table lookups above are in flight --
        // fire-and-forget device atomics, issued as the search goes, not at its end (8,000 of them from all workgroups' exits
        // into one cache line put 1.5 us on the end of every search).  Only the candidates of the grid's first row and first
        // column do this: between them they show every render and every warp once.
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
    const float a1 = __shfl(x, 0, 64), a3 = __shfl(x, 32, 64);
    float a2 = __shfl(x, 16, 64);
    if (frame_sum) {  // (scalar: the sum lives in an SGPR across the next candidate's pixels)
        if (kept) a2 = *frame_sum;
        else *frame_sum = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(a2)));
    }
    if (a.dbg_h1 && lane < 64) {
        for (int t = lane; t < kBins; t += 64) {
            a.dbg_h1[t] = lds.hist_render[t];
            if (a.dbg_h2) a.dbg_h2[t] = lds.hist_warped[t];
        }
    }
    if (lane == 0) commit_score(a, p, w, s, a1, a2, a3, prev_key);
}

// End of a workgroup of nmi_grid_kernel, by all of wavefront 0: publish_winner (nmi_device.h) plus the content probe's share.
// The workgroup that draws the last ticket fetches the plan's bins-seen masks (final_phase ORs them in; it zeroes them for
// the next search) in the same round trip as the final key, posts the winner first and then (nr, nw) to the pinned word
// the context watches.  Nothing waits for the ORs of other workgroups: a straggling OR can cost a bin in this count or add
// one to the next search's -- the count is a hint for the host's choice of kernels, every few-levels launch probes its own
// stacks exactly.
// `expected`: workgroups of the launch that call this (all of them: gridDim.x; nmi_pix_kernel: the candidates' owners).
__device__ __forceinline__ void finish_search(const GridArgs &a, int lane, unsigned long long prev_key, uint32_t expected)
{
    LevelPlan *plan = const_cast<LevelPlan *>(a.plan);
    uint32_t arrived = 0;
    if (lane == 0) {
        const unsigned int one = prev_key == ~0ull ? 2u : 1u;  // always 1; ties the ticket to this workgroup's maxes (publish_winner)
        arrived = __hip_atomic_fetch_add(a.done, one, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (__builtin_amdgcn_readfirstlane(arrived) != expected - 1) return;
    unsigned long long final_key = 0;
    uint32_t bits = 0;
    unsigned long long *post = nullptr;
    uint32_t state = 0, max_joint = 0;
    if (lane == 0) final_key = __hip_atomic_load(a.key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (plan && lane < 32) bits = __hip_atomic_exchange(&plan->seen[lane], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (plan && lane == 0) post = plan->seen_post, state = plan->seen_state, max_joint = plan->seen_max_joint;  // (one round trip for all of them)
    if (lane == 0) {
        __hip_atomic_store(a.done, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (a.out_key) __hip_atomic_store(a.out_key, final_key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        if (a.mailbox)
            __hip_atomic_store(&a.mailbox->word, final_key | ((unsigned long long)(a.seq & 1u) << 63), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    if (plan) {
        const uint32_t n = row_sum_16((uint32_t)__popc(bits));  // lanes 0 / 16: bins seen in the render / frame marginals
        const uint32_t nw = (uint32_t)__shfl((int)n, 16, 64);
        // Only a CHANGE of the verdict goes to the host: a store to pinned host memory holds the end of the kernel back by a trip
        // over PCIe (0.8 us on every search, measured), and the host has no use for a confirmation.
        const uint32_t few = (n > 0u && nw > 0u && n * nw <= max_joint) ? 1u : 0u;
        if (lane == 0 && post && few != state) {
            plan->seen_state = few;
            // the word's upper half only has to differ from the previous post's: the 100 MHz clock serves (no counter to load)
            const uint32_t stamp = 0x80000000u | (uint32_t)wall_clock64();
            __hip_atomic_store(post, ((unsigned long long)stamp << 32) | ((unsigned long long)n << 16) | nw, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

// One candidate start to finish on the exact path (returning atomics + wrap bookkeeping + flat-region folding), all 16
// wavefronts.  It runs only for candidates with a bin above 65535 hits; the kernels call it from a separate cold loop
// AFTER their hot loop, never inside it: inlined into the hot loop it cost ~10 % there (spills, code size), and as a
// real function call inside the loop ~25 %.  Uses the parity-0 event list / total and leaves them, hist_warped and
// the joint counters zero.
template <bool SHIFTED, bool BG = true, bool ROWS = false>
__device__ __forceinline__ void exact_candidate(Lds &lds, const GridArgs &a, int tid, int p, unsigned long long &prev_key)
{
    const int lane = tid & 63, wave = tid >> 6;
    const int w = p / a.S_local, s = p - w * a.S_local;
    __syncthreads();  // wavefront 0 may still be finishing the previous candidate's final phase (it resets shared state)
    histogram_phase<true, SHIFTED, 1, kBlock, true, ROWS>(lds, 0, a, a.render_stack + (size_t)s * a.npix, a.warp_stack + (size_t)w * a.npix, tid, 0,
                                                          ROWS ? a.height * a.chunks_per_row : a.npix >> 4);
    __syncthreads();
    decode_phase<!BG>(lds, 0, a, wave, lane);
    __syncthreads();
    if (wave == 0) {
        final_phase(lds, a, lane, p, w, s, prev_key);
        for (int t = lane; t < kBins; t += 64) lds.hist_warped[t] = 0;
        if (lane == 0) lds.ovf_n[0] = lds.total[0] = 0;
        if (lane < kSide) lds.side_key[0][lane] = lds.side_cnt[0][lane] = 0;
    }
    __syncthreads();
}

}  // namespace

}  // namespace nmi
