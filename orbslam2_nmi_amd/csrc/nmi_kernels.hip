// nmi_kernels.hip -- gfx950 (MI355X / CDNA4) kernels of the NMI pose-candidate scoring path.
//
// What is computed is fixed by the reference (gsanya/orbslam2_NMI, paths relative to its root):
//   Thirdparty/CUDA_Functions/NMI.cu:42-104   joint + marginal 256-bin histograms of (render, warped frame)
//   Thirdparty/CUDA_Functions/NMI.cu:230-267  per-bin term  (c/len) * log2f(c/len), len = W*H
//   Thirdparty/CUDA_Functions/NMI.cu:270-339  stride-halving fp32 trees (joint rows first, then row sums)
//   Thirdparty/CUDA_Functions/NMI.cu:342-362  SUC / ENMI score with the all-zero guard
//   Thirdparty/Localization/helperFunctions.cpp:50-103  arg-max (strict '>' from 0, lowest index on ties)
// How it is computed is new: one 1024-lane workgroup per pose candidate owns the whole
// 256x256 joint histogram in LDS as packed 16-bit counters (129 KiB of the CU's 160 KiB: rows 129 words apart); counts above 65535
// are caught by a pixel-count test and redone with exact wrap bookkeeping; the entropy terms come from a
// per-context table indexed by count; the trees are evaluated in registers / DPP in the reference's order; the
// score, the rating-table store and the arg-max (one 64-bit atomicMax per candidate) are fused into the
// same launch.  Also here: the warp-stack and point-cloud render-stack producers.
// Histogramming is integer scatter work: no MFMA.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nmi_grid_device.h"

namespace nmi {

// One workgroup per candidate (grid-stride over the candidates of this launch).
//
// HIST = 3 (default with BG on): the histogram phase uses non-returning atomics and no wrap test; the
// decode phase sums every decoded counter, and since a wrapped 16-bit field always loses weight
// (a low wrap turns 65536 hits into one carry, a high wrap drops 65536), the sum equals the pixel
// count iff no field wrapped.  A candidate that fails the test is simply histogrammed again with the
// exact wrap bookkeeping (HIST = 1 path); only frames with a bin above 65535 hits ever pay that.
//
// Two barriers per candidate: B1 histogram -> decode, B2 decode -> (wavefront 0: three final trees +
// score + arg-max) || (all other wavefronts: next candidate's histogram phase).  The small per-candidate
// state that the two sides would share is double-buffered by candidate parity.
//
// nmi_kernels_gated.hip compiles this file a second time with NMI_GRID_KERNEL_GATED defined: the same kernel under the
// name nmi_grid_kernel_gated, which returns at once unless the few-levels kernels enqueued before it handed the search
// back (plan->use == 0, nmi_fewlevels_kernel.hip).  A second translation unit rather than a template parameter because
// this kernel sits at its register cap: the mere presence of more instantiations in this unit changed its allocation.
//
// nmi_kernels_stamped.hip compiles it a third time (NMI_GRID_KERNEL_STAMPED) as nmi_grid_kernel_stamped: the same code plus
// wall-clock stamps of one candidate of every workgroup -- its k-th, k = stamp_params.k, 0 by default -- at the phase
// boundaries (NMI_OPT_STAMPS, NMI_OPT_STAMP_CANDIDATE, tools/grid_stamps.py).  In that unit the wavefronts' pixel shares
// (slab_cum, nmi_grid_device.h) are a device variable that NMI_OPT_WAVE_SHARES overwrites: the calibration runs.
#if defined(NMI_GRID_KERNEL_GATED)
#define NMI_GRID_KERNEL_NAME nmi_grid_kernel_gated
#elif defined(NMI_GRID_KERNEL_STAMPED)
#define NMI_GRID_KERNEL_NAME nmi_grid_kernel_stamped
#elif defined(NMI_GRID_KERNEL_ROWS)
#define NMI_GRID_KERNEL_NAME nmi_grid_kernel_rows
#else
#define NMI_GRID_KERNEL_NAME nmi_grid_kernel
#endif
#ifdef NMI_GRID_KERNEL_STAMPED
#define NMI_GRID_STAMP(k)                                                                                         \
    do {                                                                                                          \
        if (a.dbg_stamps && tid == ((k) == 7 ? 64 : 0) && stamp_on) a.dbg_stamps[blockIdx.x * 8 + (k)] = wall_clock64(); \
    } while (0)
#else
#define NMI_GRID_STAMP(k) \
    do {                  \
    } while (0)
#endif
#ifndef NMI_WAVE_SLABS
#define NMI_WAVE_SLABS 1  // 0: equal pixel shares for all wavefronts, as before the slabs (timing comparisons only)
#endif
#ifdef NMI_GRID_KERNEL_STAMPED
namespace {
__device__ uint32_t stamp_candidate = 0;  // which candidate of every workgroup is stamped (its k-th)
}
#endif
template <bool BG, bool SHIFTED, int HIST>
__global__ __launch_bounds__(NMI_BLOCK_THREADS) void NMI_GRID_KERNEL_NAME(GridArgs a)
{
    __shared__ Lds lds;
#ifdef NMI_GRID_KERNEL_GATED
    if (a.plan->use != 0u) return;
#endif
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
#ifdef NMI_GRID_KERNEL_STAMPED
    bool stamp_on = true;  // inside the loop: the workgroup's k-th candidate only
    const int stamp_ordinal = slot_in_round(blockIdx.x, gridDim.x) + (int)stamp_candidate * (int)gridDim.x;
#endif
    NMI_GRID_STAMP(0);
    constexpr bool kOptimistic = HIST == 3;
    constexpr int kFirst = kOptimistic ? 2 : HIST;
#ifdef NMI_GRID_KERNEL_ROWS
    constexpr bool kRows = true;  // rows that are not whole aligned chunks (histogram_phase)
#define NMI_ALL_CHUNKS (a.height * a.chunks_per_row)
#else
    constexpr bool kRows = false;
#define NMI_ALL_CHUNKS (a.npix >> 4)
#endif
    // Background rule off (NMI.cu:85) on the optimistic path: every pixel is counted, so that the wrap detector knows the
    // expected total (W*H), and decode_phase clears the row and the column of intensity 0 -- the skipped pixels.  Only
    // with 256 bins: the rule looks at the intensity before the shift, and bin 0 of a shifted histogram also holds
    // intensities 1 .. 2^shift - 1 (launch_grid sends BG off + shift to the exact path, HIST = 1).
    constexpr bool kZero0 = !BG && kOptimistic && !SHIFTED;
    constexpr bool kCountAll = BG || kZero0;
    // Pixel shares by wavefront age (histogram_phase) where the fast loop runs; the exact-only instantiations (HIST = 1: careful
    // loop from the first chunk, cold) keep equal shares, like exact_candidate -- the slabs cost them up to 60 bytes of scratch.
    constexpr bool kSlabs = NMI_WAVE_SLABS != 0 && kFirst == 2;
    // A workgroup keeps its warp (the host's visiting order sees to that, build_search_order): with every pixel counted the frame
    // marginal and its entropy sum are the warp image's alone, so only the first of a run of candidates on one warp forms them
    // (decode_phase<.., true>, final_phase's `kept`).  Not with the background rule off (the skipped pixels depend on the render),
    // not while a debug export wants every candidate's marginal, and not for a candidate the content probe reads the frame
    // marginal of (s == 0).  Every candidate this loop has scored passed the wrap test, so what is kept is exact; the cold loop
    // below forms everything per candidate.
    constexpr bool kKeepWarp = kOptimistic && BG;

    if (blockIdx.x == 0 && tid == 0 && a.reset_key) *a.reset_key = 0ull;  // next launch's slot; idle during this one
    // The LDS copy of the term table is first needed by the first decode phase: fetch it now, park it in
    // registers across the first histogram phase, store it before the first barrier.
    float tab[kLdsTable / kBlock];
#pragma unroll
    for (int k = 0; k < kLdsTable / kBlock; ++k) {
        const int c = tid + k * kBlock;
        tab[k] = a.table[c <= a.npix ? c : 0];
    }
    {
        uint4 *j4 = reinterpret_cast<uint4 *>(lds.joint);
        const uint4 z = {0, 0, 0, 0};
        for (int i = tid; i < kJointWords / 4; i += kBlock) j4[i] = z;
    }
    if (tid < kBins) lds.hist_warped[tid] = 0;
    if (tid < 2) lds.ovf_n[tid] = lds.total[tid] = 0;
    if (tid < 2 * kSide) (&lds.side_key[0][0])[tid] = (&lds.side_cnt[0][0])[tid] = 0;
    bool table_pending = true;
    int exact_from = -1;  // first ordinal of this workgroup that needs the exact path (workgroup-uniform)
    __syncthreads();
    NMI_GRID_STAMP(1);

    const int total = a.S_local * a.Wn;
    unsigned long long prev_key = 0;
    int par = 0;
    int kept_w = -1;         // the warp whose frame marginal sum is in frame_sum (workgroup-uniform)
    float frame_sum = 0.0f;  // (wavefront 0)
    const bool keep_ok = kKeepWarp && !a.dbg_h1 && !a.dbg_h2;
    const int slot = slot_in_round(blockIdx.x, gridDim.x);
    int ordinal = slot;  // this workgroup visits ordinals slot, slot + grid, slot + 2 grid, ...
    for (; ordinal < total; ordinal += gridDim.x, par ^= 1) {
        const int p = candidate_at(a, ordinal);
        const int w = p / a.S_local;
        const int s = p - w * a.S_local;
        const uint8_t *render = a.render_stack + (size_t)s * a.npix;
        const uint8_t *warped = a.warp_stack + (size_t)w * a.npix;
#ifdef NMI_GRID_KERNEL_STAMPED
        stamp_on = ordinal == stamp_ordinal;
#endif
        NMI_GRID_STAMP(7);  // wavefront 1 starts on this candidate's pixels (wavefront 0 may have had the previous one to score)

        if (a.phase_mask & 1) {
            if (a.phase_mask & 8) {  // ablation: only half of the wavefronts take part in the histogram phase
                if (wave < kWaves / 2) histogram_phase<kCountAll, SHIFTED, kFirst, kBlock / 2, true, kRows>(lds, par, a, render, warped, tid, 0, NMI_ALL_CHUNKS);
            } else
                histogram_phase<kCountAll, SHIFTED, kFirst, kBlock, true, kRows, kSlabs>(lds, par, a, render, warped, tid, 0, NMI_ALL_CHUNKS, ordinal != slot);
        }
        if (table_pending) {
#pragma unroll
            for (int k = 0; k < kLdsTable / kBlock; ++k) lds.table[tid + k * kBlock] = tab[k];
            table_pending = false;
        }
        NMI_GRID_STAMP(2);  // this wavefront's share of the pixels done
#ifdef NMI_GRID_KERNEL_STAMPED
        // ... and every wavefront's, behind the [workgroups][8] block: [workgroups][16]
        if (a.dbg_stamps && lane == 0 && stamp_on) a.dbg_stamps[gridDim.x * 8 + blockIdx.x * 16 + wave] = wall_clock64();
#endif
        __syncthreads();  // B1
        NMI_GRID_STAMP(3);
        const bool kept = keep_ok && w == kept_w && !(s == 0 && a.plan);
        if (a.phase_mask & 2) {
            if (kKeepWarp && kept) decode_phase<false, true>(lds, par, a, wave, lane);
            else decode_phase<kZero0>(lds, par, a, wave, lane);
        }
        kept_w = w;
        __syncthreads();  // B2
        NMI_GRID_STAMP(4);
        if (kOptimistic && (a.phase_mask & 3) == 3 && lds.total[par] != (uint32_t)a.npix) {
            // Some counter wrapped (workgroup-uniform, rare).  This candidate and, since the same frame and renders
            // come back, all later ones of this workgroup are scored on the exact path in the cold loop below.
            exact_from = ordinal;
            break;
        }
        if (wave == 0) {
            if (a.phase_mask & 2) final_phase(lds, a, lane, p, w, s, prev_key, kept, kKeepWarp ? &frame_sum : nullptr);
            if (!kept)
                for (int t = lane; t < kBins; t += 64) lds.hist_warped[t] = 0;
            if (lane == 0) {
                lds.ovf_n[par] = 0;       // consumed by this candidate's decode; next used two candidates on
                lds.total[par ^ 1] = 0;   // read by everyone right after the previous B2; next candidate adds to it
            }
            if (lane < kSide) {  // like ovf_n[par]
                int l = lane;
                asm volatile("" : "+v"(l));  // keep the two addresses out of long-lived (spilled) registers
                lds.side_key[par][l] = lds.side_cnt[par][l] = 0;
            }
        }
        NMI_GRID_STAMP(5);  // score committed (wavefront 0)
    }

    if (kOptimistic && exact_from >= 0) {
        __syncthreads();  // everyone has read the failed total; wavefront 0 is past the previous candidate's final phase
        if (tid < kBins) lds.hist_warped[tid] = 0;
        if (tid < 2) lds.total[tid] = lds.ovf_n[tid] = 0;
        if (tid < 2 * kSide) (&lds.side_key[0][0])[tid] = (&lds.side_cnt[0][0])[tid] = 0;
        __syncthreads();
        for (int o = exact_from; o < total; o += gridDim.x) exact_candidate<SHIFTED, !kZero0, kRows>(lds, a, tid, candidate_at(a, o), prev_key);
    }

    if (wave == 0 && !(a.phase_mask & 16)) {  // bit 4: timing experiment without the protocol (no result)
        finish_search(a, lane, prev_key, gridDim.x);
    }
#ifdef NMI_GRID_KERNEL_STAMPED
    stamp_on = true;
#endif
    NMI_GRID_STAMP(6);
}

#if defined(NMI_GRID_KERNEL_ROWS)
hipError_t launch_grid_rows(const GridArgs &a, int workgroups, bool use_bg, hipStream_t stream)
{
    if (a.width < 32 || (a.hist_variant != 1 && a.hist_variant != 3)) return hipErrorInvalidValue;
    const dim3 grid(workgroups), block(kBlock);
    const bool exact_only = a.hist_variant == 1 || (!use_bg && a.shift != 0);  // (as launch_grid: BG off below 256 bins has no optimistic path)
    if (exact_only) {
        if (use_bg) {
            if (a.shift != 0) hipLaunchKernelGGL((nmi_grid_kernel_rows<true, true, 1>), grid, block, 0, stream, a);
            else hipLaunchKernelGGL((nmi_grid_kernel_rows<true, false, 1>), grid, block, 0, stream, a);
        } else {
            if (a.shift != 0) hipLaunchKernelGGL((nmi_grid_kernel_rows<false, true, 1>), grid, block, 0, stream, a);
            else hipLaunchKernelGGL((nmi_grid_kernel_rows<false, false, 1>), grid, block, 0, stream, a);
        }
    } else if (a.shift != 0) {
        hipLaunchKernelGGL((nmi_grid_kernel_rows<true, true, 3>), grid, block, 0, stream, a);
    } else if (use_bg) {
        hipLaunchKernelGGL((nmi_grid_kernel_rows<true, false, 3>), grid, block, 0, stream, a);
    } else {
        hipLaunchKernelGGL((nmi_grid_kernel_rows<false, false, 3>), grid, block, 0, stream, a);
    }
    return hipGetLastError();
}
#elif defined(NMI_GRID_KERNEL_STAMPED)
// tools only: 256 bins, background rule on, default histogram variant
// NMI_OPT_STAMP_CANDIDATE / NMI_OPT_WAVE_SHARES: k, and (or nullptr) the two rows of 17 cumulative Q16 shares that replace slab_cum
// in this unit's kernel, for the current device.  Blocking.
hipError_t set_stamped_experiment(int k, const uint32_t *cum)
{
    const uint32_t kk = (uint32_t)k;
    hipError_t e = hipMemcpyToSymbol(HIP_SYMBOL(stamp_candidate), &kk, sizeof kk);
    if (e == hipSuccess && cum) {
        for (int r = 0; r < 2; ++r)
            for (int v = 0; v <= kWaves; ++v) {
                const uint32_t c = cum[r * (kWaves + 1) + v];
                if (c > 65536u || (v == 0 && c != 0u) || (v == kWaves && c != 65536u) || (v > 0 && c < cum[r * (kWaves + 1) + v - 1])) return hipErrorInvalidValue;
            }
        e = hipMemcpyToSymbol(HIP_SYMBOL(slab_cum), cum, 2 * (kWaves + 1) * sizeof(uint32_t));
    }
    return e;
}

hipError_t launch_grid_stamped(const GridArgs &a, int workgroups, hipStream_t stream)
{
    if (a.hist_variant != 3 || a.shift != 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL((nmi_grid_kernel_stamped<true, false, 3>), dim3(workgroups), dim3(kBlock), 0, stream, a);
    return hipGetLastError();
}
#elif defined(NMI_GRID_KERNEL_GATED)
// The fallback launch behind launch_fewlevels: 256 bins, default histogram variant.
hipError_t launch_grid_gated(const GridArgs &a, int workgroups, bool use_bg, hipStream_t stream)
{
    if (a.hist_variant != 3 || !a.plan || (a.shift != 0 && !use_bg)) return hipErrorInvalidValue;
    const dim3 grid(workgroups), block(kBlock);
    if (a.shift != 0)
        hipLaunchKernelGGL((nmi_grid_kernel_gated<true, true, 3>), grid, block, 0, stream, a);
    else if (use_bg)
        hipLaunchKernelGGL((nmi_grid_kernel_gated<true, false, 3>), grid, block, 0, stream, a);
    else
        hipLaunchKernelGGL((nmi_grid_kernel_gated<false, false, 3>), grid, block, 0, stream, a);
    return hipGetLastError();
}
#else  // everything below belongs to the primary translation unit only

#ifdef NMI_BUILD_ABLATIONS  // experiments kept for tools/ablate.py; not part of the shipped library (profiles/NOTES.md)
// ---------------------------------------------------------------------------------------------------------
// Pipelined ("wavefront-specialised") form of the same computation (NMI_OPT_HIST_VARIANT = 4, experimental).
// Exact, covered by the parity tests, but measured SLOWER than the sequential kernel on MI355X (114 vs 95 us per 729
// candidates): the decode wavefronts take issue slots from the histogram wavefronts, 8 histogram wavefronts add
// pixels 22 % slower than 16, and the drain is a third serial step.  Kept as an ablation; see profiles/NOTES.md.
//
// The histogram phase is bound by the LDS atomic unit, the decode arithmetic by VALU issue and latency; run one
// after the other (kernel above) a CU leaves each unit idle in turn.  Here the 16 wavefronts split into
//   H = wavefronts 0..7   histogram phase of candidate k (non-returning atomics into the packed LDS joint)
//   D = wavefronts 8..15  decode arithmetic of candidate k-1 (terms, trees, marginals) from its drained counters
// with two workgroup barriers per candidate: X (histogram k and arithmetic k-1 done) and Y (all wavefronts have
// drained candidate k's packed counters from LDS to the workgroup's scratch slab in L2 and cleared the LDS words;
// meanwhile wavefront 0 forms the score of k-1).  D then reads candidate k back from the slab while H is already
// adding candidate k+1.  Only the drain (an LDS read + clear sweep with coalesced stores) stays serial with H.
// Counter wraps are detected by the pixel-count test as before; the first wrapped candidate switches the
// workgroup to the sequential exact path (below) for that candidate and all that follow.
// ---------------------------------------------------------------------------------------------------------
namespace {

constexpr int kHalf = kBlock / 2;               // lanes per role
constexpr int kDWaves = kWaves / 2;             // 8 decode wavefronts
constexpr int kDRows = kBins / kDWaves;         // 32 joint rows per decode wavefront
constexpr int kDPasses = kDRows / 4;            // 8 passes of 4 rows (one per 16-lane DPP row)

// Joint row of DPP row r in pass `pass` of decode wavefront `dwave`: the two rows of a 32-lane LDS access group are 16 apart
// (opposite halves of the banks under the 129-word row stride, nmi_grid_device.h).
__device__ __forceinline__ int ws_row(int dwave, int pass, int r) { return dwave * kDRows + (r & 1) * 16 + pass * 2 + (r >> 1); }

// Drain, all 16 wavefronts: packed counters LDS -> this workgroup's scratch slab in global memory (it stays in L2),
// clearing the LDS words.  The slab is written in the order the decode wavefronts read it -- [dwave][pass][k][lane],
// 256 contiguous bytes per wavefront instruction -- with the word ownership of decode_phase (lane i of a 16-lane row
// owns words i + 16*k of its joint row) and the rows of ws_row.
__device__ __forceinline__ void drain_to_scratch(Lds &lds, uint32_t *__restrict__ slab, int wave, int lane)
{
    const int i = lane & 15, r = lane >> 4;
    const int dwave = wave >> 1, pass0 = (wave & 1) * (kDPasses / 2);
#pragma unroll
    for (int pp = 0; pp < kDPasses / 2; ++pp) {
        const int pass = pass0 + pp;
        const int d1 = ws_row(dwave, pass, r);
        uint32_t wd[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const uint32_t idx = decode_word(d1, i, k);
            wd[k] = lds.joint[idx];
            lds.joint[idx] = 0;
        }
        uint32_t *dst = slab + ((dwave * kDPasses + pass) * 8) * 64 + lane;
#pragma unroll
        for (int k = 0; k < 8; ++k) dst[k * 64] = wd[k];
    }
}

// D: per-bin terms, row trees, marginals for the 32 rows of this decode wavefront, read back from the slab
// (agent-scope loads: the slab was written by other wavefronts of this CU through L2, this CU's L1 may hold the
// lines of an earlier candidate).  The next pass's words are in flight while the current pass is reduced.
__device__ __forceinline__ void load_pass(const uint32_t *__restrict__ src, uint32_t (&wd)[8])
{
#pragma unroll
    for (int k = 0; k < 8; ++k) wd[k] = __hip_atomic_load(src + k * 64, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ void decode_pass(Lds &lds, const GridArgs &a, int d1, int i, const uint32_t (&wd)[8],
                                            uint32_t (&col_lo)[8], uint32_t (&col_hi)[8], uint32_t &wave_total)
{
    uint32_t lo[8], hi[8], rsum = 0, cmax = 0;
    float tl[8], th[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        lo[k] = wd[k] & 0xFFFFu;
        hi[k] = wd[k] >> 16;
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
            if (lo[k] >= (uint32_t)kLdsTable) tl[k] = a.table[lo[k]];
            if (hi[k] >= (uint32_t)kLdsTable) th[k] = a.table[hi[k]];
        }
    }
    rsum = row_sum_16(rsum);
    wave_total += rsum;
    const float x = row_tree_16(lane_tree_16(tl, th));
    if (i == 0) {
        lds.hist_render[d1] = rsum;
        lds.joint_row_sums[d1] = x;
    }
}

__device__ __forceinline__ void decode_from_scratch(Lds &lds, const GridArgs &a, const uint32_t *__restrict__ slab, int dwave,
                                                    int lane)
{
    const int i = lane & 15, r = lane >> 4;
    uint32_t col_lo[8], col_hi[8], wave_total = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) col_lo[k] = col_hi[k] = 0;
    const uint32_t *src = slab + (dwave * kDPasses * 8) * 64 + lane;
    uint32_t wa[8], wb[8];
    load_pass(src, wa);
#pragma unroll 1
    for (int pass = 0; pass < kDPasses; pass += 2) {
        load_pass(src + (pass + 1) * 8 * 64, wb);
        decode_pass(lds, a, ws_row(dwave, pass, r), i, wa, col_lo, col_hi, wave_total);
        if (pass + 2 < kDPasses) load_pass(src + (pass + 2) * 8 * 64, wa);
        decode_pass(lds, a, ws_row(dwave, pass + 1, r), i, wb, col_lo, col_hi, wave_total);
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

template <bool SHIFTED>
__global__ __launch_bounds__(NMI_BLOCK_THREADS) void nmi_grid_kernel_ws(GridArgs a)
{
    __shared__ Lds lds;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const bool is_hist = wave < kDWaves;  // wavefront-uniform role
    const int dwave = wave - kDWaves;

    if (blockIdx.x == 0 && tid == 0 && a.reset_key) *a.reset_key = 0ull;
    {
        uint4 *j4 = reinterpret_cast<uint4 *>(lds.joint);
        const uint4 z = {0, 0, 0, 0};
        for (int i = tid; i < kJointWords / 4; i += kBlock) j4[i] = z;
    }
    for (int c = tid; c < kLdsTable; c += kBlock) lds.table[c] = a.table[c <= a.npix ? c : 0];
    if (tid < kBins) lds.hist_warped[tid] = 0;
    if (tid < 2) lds.ovf_n[tid] = lds.total[tid] = 0;
    if (tid < 2 * kSide) (&lds.side_key[0][0])[tid] = (&lds.side_cnt[0][0])[tid] = 0;
    if (tid == 0) lds.fallback = lds.redo_n = 0;
    __syncthreads();

    const int total = a.S_local * a.Wn;
    const int slot = slot_in_round(blockIdx.x, gridDim.x);
    const int n = slot < total ? (total - slot + (int)gridDim.x - 1) / (int)gridDim.x : 0;  // candidates of this workgroup
    unsigned long long prev_key = 0;
    // two slabs per workgroup, alternating by candidate: D reads slab (k-1)&1 while the drain of candidate k fills slab k&1
    uint32_t *const slab0 = a.scratch + (size_t)blockIdx.x * 2 * kWords;

    int k = 0;        // stage: H works on candidate k, D on candidate k-1
    bool bail = false;
    for (; k <= n && !bail; ++k) {
        const int p = k < n ? candidate_at(a, slot + k * (int)gridDim.x) : 0;
        if (is_hist) {
            if (k < n && (a.phase_mask & 1)) {
                const int w = p / a.S_local, s = p - w * a.S_local;
                histogram_phase<true, SHIFTED, 2, kHalf, false>(lds, 0, a, a.render_stack + (size_t)s * a.npix,
                                                         a.warp_stack + (size_t)w * a.npix, tid, 0, a.npix >> 4);
            }
        } else if (k > 0 && (a.phase_mask & 2)) {
            decode_from_scratch(lds, a, slab0 + ((k - 1) & 1) * kWords, dwave, lane);
        }
        __syncthreads();  // X
        if (k < n && !(a.phase_mask & 4)) drain_to_scratch(lds, slab0 + (k & 1) * kWords, wave, lane);
        if (is_hist) {
            if (wave == 0 && k > 0) {
                const int pp = candidate_at(a, slot + (k - 1) * (int)gridDim.x), w = pp / a.S_local, s = pp - w * a.S_local;
                if ((a.phase_mask & 7) == 3 && lds.total[0] != (uint32_t)a.npix) {
                    // a 16-bit counter wrapped in candidate k-1: hand it (and everything after it) to the exact path
                    if (lane == 0) {
                        lds.fallback = 1;
                        lds.redo[lds.redo_n++] = (uint32_t)(k - 1);
                    }
                } else {
                    final_phase(lds, a, lane, pp, w, s, prev_key);
                }
                for (int t = lane; t < kBins; t += 64) lds.hist_warped[t] = 0;
                if (lane == 0) lds.total[0] = 0;
            }
        }
        __builtin_amdgcn_s_waitcnt(0);  // the slab stores of this wavefront have reached L2 before anyone is released
        __syncthreads();  // Y
        bail = lds.fallback != 0;
    }

    if (bail) {
        // Stage k-1 detected the wrap; candidate k-1 (if any) has already been drained into the D registers.
        const int kd = k - 1;  // ordinal of the drained candidate
        if (kd < n) {
            if (!is_hist) decode_from_scratch(lds, a, slab0 + (kd & 1) * kWords, dwave, lane);
            __syncthreads();
            if (wave == 0) {
                const int pp = candidate_at(a, slot + kd * (int)gridDim.x), w = pp / a.S_local, s = pp - w * a.S_local;
                if (lds.total[0] != (uint32_t)a.npix) {
                    if (lane == 0) lds.redo[lds.redo_n++] = (uint32_t)kd;
                } else {
                    final_phase(lds, a, lane, pp, w, s, prev_key);
                }
                for (int t = lane; t < kBins; t += 64) lds.hist_warped[t] = 0;
                if (lane == 0) lds.total[0] = 0;
            }
            __syncthreads();
        }
        const int nredo = (int)lds.redo_n;
        for (int e = 0; e < nredo; ++e)
            exact_candidate<SHIFTED>(lds, a, tid, candidate_at(a, slot + (int)lds.redo[e] * (int)gridDim.x), prev_key);
        for (int kk = kd + 1; kk < n; ++kk) exact_candidate<SHIFTED>(lds, a, tid, candidate_at(a, slot + kk * (int)gridDim.x), prev_key);
    }

    if (tid == 0) publish_winner(a, prev_key);
}

#endif  // NMI_BUILD_ABLATIONS

// table[c] = (c/len) * log2(c/len) in the reference's fp32 form (NMI.cu:245): p = fl32(c/len),
// l = log2 of p rounded once to fp32 (evaluated in fp64 so the rounding is the correct one; CUDA's
// and glibc's log2f are each within 1 ulp of it), term = fl32(p * l).
__global__ void nmi_table_kernel(float *table, int npix)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c > npix) return;
    if (c == 0) {
        table[0] = 0.0f;
        return;
    }
    const float p = (float)c / (float)npix;
    const float l = (float)log2((double)p);
    table[c] = p * l;
}

hipError_t launch_table(float *table, int npix, hipStream_t stream)
{
    const int threads = 256;
    const int blocks = (npix + 1 + threads - 1) / threads;
    hipLaunchKernelGGL(nmi_table_kernel, dim3(blocks), dim3(threads), 0, stream, table, npix);
    return hipGetLastError();
}

template <int HIST>
static void launch_hist(const GridArgs &a, dim3 grid, dim3 block, bool use_bg, hipStream_t stream)
{
    const bool shifted = a.shift != 0;
    if (use_bg) {
        if (shifted)
            hipLaunchKernelGGL((nmi_grid_kernel<true, true, HIST>), grid, block, 0, stream, a);
        else
            hipLaunchKernelGGL((nmi_grid_kernel<true, false, HIST>), grid, block, 0, stream, a);
    } else {
        if (shifted)
            hipLaunchKernelGGL((nmi_grid_kernel<false, true, HIST>), grid, block, 0, stream, a);
        else
            hipLaunchKernelGGL((nmi_grid_kernel<false, false, HIST>), grid, block, 0, stream, a);
    }
}

hipError_t launch_grid(const GridArgs &a, int workgroups, bool use_bg, hipStream_t stream)
{
    dim3 grid(workgroups), block(kBlock);
    // rows that are not whole aligned 16-byte chunks: the unaligned-row form instead of the byte path (frames under 32 pixels
    // of width keep the byte path)
    if (!a.vec_ok && a.width >= 32 && (a.hist_variant == 1 || a.hist_variant == 3) && !(a.phase_mask & 8)) return launch_grid_rows(a, workgroups, use_bg, stream);
    switch (a.hist_variant) {
    case 1: launch_hist<1>(a, grid, block, use_bg, stream); break;
    case 3:
        if (a.dbg_stamps && use_bg && a.shift == 0) return launch_grid_stamped(a, workgroups, stream);  // tools/grid_stamps.py
        // The wrap detector of HIST = 3 needs the expected pixel count: W*H with BG on, and with BG off at 256 bins (the
        // kernel then counts every pixel and clears row / column 0 afterwards); BG off with fewer bins takes the exact path.
        if (use_bg || a.shift == 0)
            launch_hist<3>(a, grid, block, use_bg, stream);
        else
            launch_hist<1>(a, grid, block, use_bg, stream);
        break;
#ifdef NMI_BUILD_ABLATIONS
    case 0: launch_hist<0>(a, grid, block, use_bg, stream); break;
    case 2: launch_hist<2>(a, grid, block, use_bg, stream); break;
    case 4:
        // pipelined kernel (experimental).  It has no debug exports and needs BG on.
        if (use_bg && !a.dbg_joint && !a.dbg_h1 && !a.dbg_h2 && !a.dbg_sums) {
            if (a.shift != 0)
                hipLaunchKernelGGL((nmi_grid_kernel_ws<true>), grid, block, 0, stream, a);
            else
                hipLaunchKernelGGL((nmi_grid_kernel_ws<false>), grid, block, 0, stream, a);
        } else if (use_bg) {
            launch_hist<3>(a, grid, block, use_bg, stream);
        } else {
            launch_hist<1>(a, grid, block, use_bg, stream);
        }
        break;
#endif
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

bool ablation_variants_built()
{
#ifdef NMI_BUILD_ABLATIONS
    return true;
#else
    return false;
#endif
}

int grid_kernel_lds_bytes() { return (int)sizeof(Lds); }
size_t grid_kernel_scratch_bytes(int workgroups) { return (size_t)workgroups * 2 * kWords * sizeof(uint32_t); }

#endif  // primary translation unit

}  // namespace nmi
