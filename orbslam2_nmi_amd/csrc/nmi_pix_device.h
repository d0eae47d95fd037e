// nmi_pix_device.h -- the pixel-range kernels' shared device code (nmi_pix_kernel.hip, nmi_masked_pix_kernel.hip,
// nmi_covered_pix_kernel.hip): which workgroup scores what (pix_unit), the dealing of the pair's pieces and their addressing
// (Deal, Pieces), clear_counters (clear_lds of nmi_grid_device.h and the heal flag), the plain and the masked dealt loops, the
// hand-off (PixHeader, unit layout, tagged mask granules; the helper's pix_publish and the owner's pix_collect), the owner's merged decode and its final trees, and the launchers' shared host code.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "nmi_grid_device.h"
#include "nmi_mask_device.h"  // masked_add_chunk, nonzero_byte_bits, both_nonzero, popc4, cover_term

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
constexpr int kMaxRanges = kPixMaxRanges;  // (nmi_search_plan.h)

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

// What a workgroup of a pixel-range launch scores.  Helpers first: blocks 0 .. total * (P - 1) - 1 are range q = 1 + b / total
// of candidate p = b % total, then come the owners (q = 0) -- see Liveness in nmi_pix_kernel.hip.
struct PixUnit {
    int total, q, p, w, s;  // candidates of the launch; this workgroup's range, candidate, warp and render
    uint32_t tag;           // the launch's tag: never 0 (the state of fresh memory); the replay word counts the replays of a
                            // captured graph, whose arguments are frozen
    char *blocks;           // the candidate's P - 1 hand-off blocks, helper q's at (q - 1) * kPixBlockBytes
};
__device__ __forceinline__ PixUnit pix_unit(const GridArgs &a, int P, const DealArgs &dealing, const uint32_t *replay)
{
    PixUnit u;
    u.total = a.S_local * a.Wn;
    const int helpers = u.total * (P - 1);
    const int b = (int)blockIdx.x;
    u.q = b < helpers ? 1 + (u.total > 1 ? (int)__umulhi((uint32_t)b, dealing.total_magic) : b) : 0;
    u.p = b < helpers ? b - (u.q - 1) * u.total : b - helpers;
    u.w = u.p / a.S_local;
    u.s = u.p - u.w * a.S_local;
    u.tag = 0x80000000u | ((a.epoch + (replay ? __hip_atomic_load(replay, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u)) & 0x7FFFFFFFu);
    u.blocks = reinterpret_cast<char *>(a.blocks) + (size_t)u.p * (size_t)(P - 1) * kPixBlockBytes;
    return u;
}

// Every counter of the workgroup to zero, before its pixels and before a candidate is scored once more on an exact path.  (The
// masked forms never set a side counter, so clearing them again before their heal stores zeros over zeros; and every thread has
// read lds.fallback before the barrier that precedes a heal's clear.)
__device__ __forceinline__ void clear_counters(Lds &lds, int tid)
{
    clear_lds(lds, tid);  // (total[0]: decoded counters; masked forms, total[1]: pixels added by all ranges)
    if (tid == 0) lds.fallback = 0;
}

// An owner's heal, counted by one thread on its way into the cold branch (kPixHeal*, nmi_kernels.h): why the candidate is scored
// once more -- the wait for a helper was given up, or the merged decode failed the count test -- and the sum nmi_pix_status
// reports, which for the plain kernel (!BOTH) has only ever held the timeouts.
__device__ __forceinline__ void pix_count_heal(uint32_t *counters, bool gave_up, bool both)
{
    if (gave_up || both) __hip_atomic_fetch_add(counters + kPixHealed, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_add(counters + (gave_up ? kPixHealTimeouts : kPixHealCountTest), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the workgroup's added pixels into *dst (LDS, zero before)
__device__ __forceinline__ void add_count(uint32_t *dst, uint32_t n, int lane)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) n += (uint32_t)__shfl_xor((int)n, off, 64);
    if (lane == 0) atomicAdd(dst, n);
}

// A workgroup's piece addressing.  Chunk c = the j-th 16-byte chunk of row y: byte y * width + 16 j of the frame and of the warp
// mask, ry * width + 16 j of the render and of its coverage mask -- rows need not be whole aligned chunks (histogram_phase's ROWS
// form, nmi_grid_device.h); the row_rem = width % 16 pixels left per row are add_row_tails' below.  Loads are clamped to the last
// chunk (a valid address); only the adds are predicated, by chunk < nchunks.
struct Pieces {
    const GridArgs &a;
    const Deal &d;
    int wave, lane, nchunks, row_rem;
    __device__ __forceinline__ Pieces(const GridArgs &a_, const Deal &d_, int wave_, int lane_)
        : a(a_), d(d_), wave(wave_), lane(lane_), nchunks(a_.height * a_.chunks_per_row), row_rem(a_.width - (a_.chunks_per_row << 4)) {}
    __device__ __forceinline__ int iters() const { return (d.n + kWaves - 1) / kWaves; }  // workgroup-uniform
    // chunk of this lane in the workgroup's iteration `it`; beyond the workgroup's pieces: some chunk >= nchunks (not added)
    __device__ __forceinline__ int chunk_of(int it) const
    {
        const int i = it * kWaves + wave;  // wavefront-uniform
        const int g = d.cnt > 1 ? (int)__umulhi((uint32_t)i, d.magic) : i;
        const int t = g * d.L + d.off + (i - g * d.cnt);
        return i < d.n ? (t << 6) + lane : 0x7FFFFFC0;
    }
    __device__ __forceinline__ uint32_t at(int c) const  // byte of chunk c in the frame (and in the warp mask: same layout)
    {
        c = min(c, nchunks - 1);
        return ((uint32_t)c << 4) + (uint32_t)__mul24((int)__umulhi((uint32_t)c, a.cpr_magic), row_rem);
    }
    __device__ __forceinline__ uint32_t rat(int c) const  // ... in the render (and in its coverage mask): NMI.cu:82, row y meets row H-1-y of a bottom-up render
    {
        c = min(c, nchunks - 1);
        const int y = (int)__umulhi((uint32_t)c, a.cpr_magic);
        const int ry = a.flip ? a.height - 1 - y : y;
        return ((uint32_t)(__mul24(y, a.flip_row) + c + a.flip_base) << 4) + (uint32_t)__mul24(ry, row_rem);
    }
};
__device__ __forceinline__ uint4 ld16(const uint8_t *base, uint32_t o) { return *reinterpret_cast<const uint4 *>(base + o); }

// The owner also adds the last width % 16 pixels of every row, one by one: those for which take(frame position, render
// position) holds.  Returns the pixels this lane added.
template <bool SHIFTED, class Take>
__device__ __forceinline__ uint32_t add_row_tails(Lds &lds, const Pieces &pc, const uint8_t *__restrict__ render, const uint8_t *__restrict__ warped, Take take)
{
    const GridArgs &a = pc.a;
    uint32_t added = 0;
    if (pc.d.off == 0 && pc.row_rem > 0) {
        const int x0 = a.chunks_per_row << 4, n = a.height * pc.row_rem;
        for (int t = pc.wave * 64 + pc.lane; t < n; t += kBlock) {
            const int y = t / pc.row_rem, x = x0 + t - y * pc.row_rem;
            const int pos = y * a.width + x, rpos = (a.flip ? a.height - 1 - y : y) * a.width + x;
            if (!take(pos, rpos)) continue;
            uint32_t d1 = render[rpos], d2 = warped[pos];
            if (SHIFTED) {
                d1 >>= a.shift;
                d2 >>= a.shift;
            }
            (void)__hip_atomic_fetch_add(&lds.joint[joint_word(d1, d2)], joint_inc(d2), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            ++added;
        }
    }
    return added;
}

// This workgroup's dealt pieces, every pixel: nmi_grid_kernel's histogram phase (non-returning atomics, flat regions folded).
template <bool SHIFTED>
__device__ __forceinline__ void histogram_dealt(Lds &lds, const GridArgs &a, const uint8_t *__restrict__ render, const uint8_t *__restrict__ warped,
                                                int wave, int lane, const Deal &d)
{
    const Pieces pc(a, d, wave, lane);
    auto ldw = [&](int c) { return ld16(warped, pc.at(c)); };
    auto ldr = [&](int c) { return ld16(render, pc.rat(c)); };
    const int nchunks = pc.nchunks, iters = pc.iters();
    (void)add_row_tails<SHIFTED>(lds, pc, render, warped, [](int, int) { return true; });
    if (iters <= 0) return;
    const bool try_flat = !(a.phase_mask & 4);
    int resume = -1;
    int c = pc.chunk_of(0);
    uint4 wa = ldw(c), ra = ldr(c), wb, rb;
    for (int it = 0; it < iters; it += 2) {
        const int cb = pc.chunk_of(it + 1);
        wb = ldw(cb);
        rb = ldr(cb);
        if (__builtin_expect(flat_hint(ra, wa), 0)) {
            resume = it;
            break;
        }
        if (c < nchunks) add_chunk<true, SHIFTED, 2, false>(lds, 0, ra, wa, a.shift, false);
        c = pc.chunk_of(it + 2);
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
        int cc = pc.chunk_of(resume);
        uint4 wc = ldw(cc), rc = ldr(cc);
#pragma unroll 1
        for (int it = resume; it < iters; ++it) {
            const int cn = pc.chunk_of(it + 1);
            const uint4 wn = ldw(cn), rn = ldr(cn);
            if (cc < nchunks) add_chunk<true, SHIFTED, 2, true>(lds, 0, rc, wc, a.shift, try_flat);
            wc = wn;
            rc = rn;
            cc = cn;
        }
    }
}

__device__ __forceinline__ uint32_t mask_popc(const uint4 &m)
{
    return __popc(nonzero_byte_bits(m.x)) + __popc(nonzero_byte_bits(m.y)) + __popc(nonzero_byte_bits(m.z)) + __popc(nonzero_byte_bits(m.w));
}

// This workgroup's dealt pieces with masks, non-returning atomics; flat chunks are not folded (fold_flat_chunk's side counters
// assume every pixel of a chunk counts).  A pixel is added where its byte of the warp's mask is nonzero and, COVERED, its byte of
// the render's coverage mask (in the render's row order) too: the covered form is the masked form whose chunk mask is
// both_nonzero of the two.  Returns the pixels this lane added.
template <bool SHIFTED, bool COVERED>
__device__ __forceinline__ uint32_t masked_histogram_dealt(Lds &lds, const GridArgs &a, const uint8_t *__restrict__ render,
                                                          const uint8_t *__restrict__ warped, const uint8_t *__restrict__ wmask,
                                                          const uint8_t *__restrict__ rmask, int wave, int lane, const Deal &d)
{
    const Pieces pc(a, d, wave, lane);
    uint32_t added = add_row_tails<SHIFTED>(lds, pc, render, warped, [&](int pos, int rpos) { return wmask[pos] != 0 && (!COVERED || rmask[rpos] != 0); });
    const int iters = pc.iters();
    if (iters <= 0) return added;
    // one chunk of prefetch (masked_histogram_phase's loop): the masks are folded after the adds, while the next loads fly
    int c = pc.chunk_of(0);
    uint32_t o = pc.at(c), ro = pc.rat(c);
    uint4 wc = ld16(warped, o), rc = ld16(render, ro), mc = ld16(wmask, o);
    if (COVERED) mc = both_nonzero(mc, ld16(rmask, ro));
#pragma unroll 1
    for (int it = 0; it < iters; ++it) {
        const int cn = pc.chunk_of(it + 1);
        o = pc.at(cn);
        ro = pc.rat(cn);
        const uint4 wn = ld16(warped, o), rn = ld16(render, ro), wmn = ld16(wmask, o), rmn = COVERED ? ld16(rmask, ro) : wmn;
        if (c < pc.nchunks) {
            added += COVERED ? popc4(mc) : mask_popc(mc);  // (both_nonzero already yields one bit per pixel)
            masked_add_chunk<true, SHIFTED, 2>(lds, 0, rc, wc, mc, a.shift);
        }
        wc = wn;
        rc = rn;
        mc = COVERED ? both_nonzero(wmn, rmn) : wmn;
        c = cn;
    }
    return added;
}

__device__ __forceinline__ int unit_offset(int wave, int kk, int lane) { return (int)sizeof(PixHeader) + ((wave * kUnitsPerLane + kk) * 64 + lane) * 16; }

// ---- the hand-off --------------------------------------------------------------------------------------------------------------
// What travels in the header beside the units is the one thing that differs between the callers.  SIDE (the plain kernel): the
// helper's flat-region side counters, merged into the owner's (side_add), or, when those are taken, onto the packed field.
// !SIDE (the masked forms, which fold nothing): the pixels the helper added, lds.total[1], in pad[0], summed into the owner's
// lds.total[1].
//
// The helper's half, called after the barrier behind its pixels: units that hold a count -> memory, write-through; the header's
// payload; drain; barrier; tagged masks.  The order matters: a granule's tag tells the owner that the units AND the payload
// are in memory, so every storing wave drains before the barrier the granules' lanes wait at.
template <bool SIDE>
__device__ __forceinline__ void pix_publish(Lds &lds, const GridArgs &a, const PixUnit &u, int wave, int lane)
{
    char *const blk = u.blocks + (size_t)(u.q - 1) * kPixBlockBytes;
    PixHeader *const hdr = reinterpret_cast<PixHeader *>(blk);
    const auto rsrc = __builtin_amdgcn_make_buffer_rsrc(blk, 0, (int)kPixBlockBytes, 0x00020000);
    const int tid = wave * 64 + lane;
    unsigned long long mask[kUnitsPerLane];
    {
        const int i = lane & 15, r = lane >> 4;
#pragma unroll
        for (int kk = 0; kk < kUnitsPerLane; ++kk) {
            const int d1 = decode_row(wave, kk >> 1, r);
            u32x4 v;
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = lds.joint[decode_word(d1, i, (kk & 1) * 4 + j)];
            const bool on = (v.x | v.y | v.z | v.w) != 0u;
            mask[kk] = __ballot(on);
            if (on) __builtin_amdgcn_raw_buffer_store_b128(v, rsrc, unit_offset(wave, kk, lane), 0, kAuxSc1);
        }
    }
    if (SIDE) {
        if (tid < kSide) {
            __hip_atomic_store(&hdr->side_key[tid], lds.side_key[0][tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&hdr->side_cnt[tid], lds.side_cnt[0][tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    } else {
        if (tid == 0) __hip_atomic_store(&hdr->pad[0], lds.total[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    uint32_t half = 0;
#pragma unroll
    for (int g = 0; g < 2 * kUnitsPerLane; ++g)
        if (lane == g) half = (uint32_t)(mask[g >> 1] >> (32 * (g & 1)));
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every storing wave, before the barrier the granules' lanes wait at
    __syncthreads();
    // (phase mask bit 9, tests only: helper 1 keeps its masks to itself, so its owner's wait must time out and heal)
    if (lane < 2 * kUnitsPerLane && !((a.phase_mask & 512) && u.q == 1))
        __hip_atomic_store(&hdr->granule[wave * 2 * kUnitsPerLane + lane], ((unsigned long long)u.tag << 32) | half, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The owner's half: the bounded wait for every helper's tag, then this lane's units of every helper, summed field by field as
// packed words into acc (a field that wraps in the sum loses weight like any other wrap), and the header's payload into the LDS.
// Called before the barrier behind the owner's pixels: the loads arrive while the slower wavefronts finish theirs.  A wave that
// gives up on a helper (kPixTimeoutTicks) sets lds.fallback and leaves acc zero.
template <bool SIDE>
__device__ __forceinline__ void pix_collect(Lds &lds, const PixUnit &u, int P, int wave, int lane, u32x4 (&acc)[kUnitsPerLane])
{
    // every wave polls for itself: lane 16 h + g the granule g of helper h + 1 that belongs to this wave's units
    unsigned long long gv = 0;
    bool seen = true;
    if (lane < 16 * (P - 1)) {
        const unsigned long long *g = reinterpret_cast<const PixHeader *>(u.blocks + (size_t)(lane >> 4) * kPixBlockBytes)->granule + wave * 16 + (lane & 15);
        unsigned long long t0 = 0;
        int tries = 0;
        while ((uint32_t)((gv = __hip_atomic_load(g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) >> 32) != u.tag) {
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
    const uint32_t gh = (uint32_t)gv;  // this lane's mask half
#pragma unroll
    for (int kk = 0; kk < kUnitsPerLane; ++kk) acc[kk] = u32x4{0, 0, 0, 0};
    if (!seen) return;
    for (int h = 0; h < P - 1; ++h) {
        const char *blk = u.blocks + (size_t)h * kPixBlockBytes;
        const auto rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<char *>(blk), 0, (int)kPixBlockBytes, 0x00020000);
        u32x4 v[kUnitsPerLane];
#pragma unroll
        for (int kk = 0; kk < kUnitsPerLane; ++kk) {
            const uint32_t lo = __builtin_amdgcn_readlane(gh, h * 16 + 2 * kk), hi = __builtin_amdgcn_readlane(gh, h * 16 + 2 * kk + 1);
            v[kk] = u32x4{0, 0, 0, 0};
            if ((((((unsigned long long)hi << 32) | lo) >> lane) & 1ull) != 0ull) v[kk] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, unit_offset(wave, kk, lane), 0, kAuxSc1);
        }
        if (SIDE) {
            if (wave == 0 && lane < kSide) {
                // a helper's side counter: into a side counter of the owner's (atomics: other wavefronts may still be folding flat
                // chunks of their own), or, when those are taken, onto the packed field (which may wrap it: the count test sees that)
                const uint32_t skey = __builtin_amdgcn_raw_buffer_load_b32(rsrc, (int)offsetof(PixHeader, side_key) + lane * 4, 0, kAuxSc1);
                const uint32_t scnt = __builtin_amdgcn_raw_buffer_load_b32(rsrc, (int)offsetof(PixHeader, side_cnt) + lane * 4, 0, kAuxSc1);
                if (skey != 0u) {
                    const uint32_t sd1 = (skey - 1u) >> 8, sd2 = (skey - 1u) & 0xFFu;
                    if (!side_add(lds, 0, sd1, sd2, scnt)) atomicAdd(&lds.joint[joint_word(sd1, sd2)], (sd2 & 128u) ? scnt << 16 : scnt);
                }
            }
        } else {
            if (wave == 0 && lane == 0) atomicAdd(&lds.total[1], __builtin_amdgcn_raw_buffer_load_b32(rsrc, (int)offsetof(PixHeader, pad), 0, kAuxSc1));
        }
#pragma unroll
        for (int kk = 0; kk < kUnitsPerLane; ++kk) acc[kk] += v[kk];
    }
}

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

// One launch of total * pix_parts workgroups (host): the dealing, the grid, and the choice among a kernel's three instantiations
// <ZERO0, SHIFTED> -- fewer than 256 bins (background rule on), 256 bins with the rule on, 256 bins with it off.
// launch(zero0, shifted, grid, dealing) enqueues the kernel; the two first arguments are std::bool_constant's.
template <class Launch>
inline hipError_t pix_launch(const GridArgs &a, int pix_parts, double owner_share, bool use_bg, Launch launch)
{
    const DealArgs g = pix_dealing(a, pix_parts, owner_share);
    const dim3 grid((unsigned)((long long)a.S_local * a.Wn * pix_parts));
    if (a.shift != 0)
        launch(std::false_type{}, std::true_type{}, grid, g);
    else if (use_bg)
        launch(std::false_type{}, std::false_type{}, grid, g);
    else
        launch(std::true_type{}, std::false_type{}, grid, g);
    return hipGetLastError();
}

// Where the owner's decode finds the term of a count at or above kLdsTable (below, lds.table has it), and what else it has:
// side counters (fold_flat_chunk's, the plain dealt loop) and the debug copy of the joint histogram.
struct TableTerms {  // a global table of npix + 1 terms: the plain and the masked kernel
    const float *table;
    uint32_t npix;
    uint32_t *dbg_joint;
    static constexpr bool kSideCounters = true;
    __device__ __forceinline__ float high(uint32_t c) const { return table[min(c, npix)]; }  // (a wrapped helper field can read high; the detector rejects the candidate)
};
struct CoverTerms {  // the candidate's own terms, evaluated (as covered_decode_phase): the covered kernel, which folds nothing and has no debug copy
    uint32_t len;
    static constexpr uint32_t *dbg_joint = nullptr;
    static constexpr bool kSideCounters = false;
    __device__ __forceinline__ float high(uint32_t c) const { return cover_term(c, len); }
};

// The owner's decode: decode_phase (ComputeEntropyKernel + AddvectorParwiseMidKernel, NMI.cu:230-287) over its own packed
// counters PLUS the helpers' (acc: their units of this lane, already summed field by field), with two differences: counters
// are not cleared (the workgroup scores one candidate) and there are no wrap events to replay (nobody used returning atomics).
template <bool ZERO0, class Terms>
__device__ __forceinline__ void decode_merged(Lds &lds, const Terms &terms, int wave, int lane, const u32x4 (&acc)[kUnitsPerLane])
{
    const bool side_any = Terms::kSideCounters && lds.side_key[0][0] != 0u;
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
                if (lo[k] >= (uint32_t)kLdsTable) tl[k] = terms.high(lo[k]);
                if (hi[k] >= (uint32_t)kLdsTable) th[k] = terms.high(hi[k]);
            }
        }
        rsum = row_sum_16(rsum);
        if (!ZERO0) wave_total += rsum;
        const float x = row_tree_16(lane_tree_16(tl, th));
        if (i == 0) {
            lds.hist_render[d1] = rsum;
            lds.joint_row_sums[d1] = x;
        }
        if (terms.dbg_joint) {
            uint32_t *row = terms.dbg_joint + d1 * kBins;
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

// final_phase (nmi_grid_device.h: the three 256-element trees of AddVectorPairwiseKernel, NMI.cu:295-339, side by side in DPP rows
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
