// nmi_grid_kernel.h -- nmi_grid_kernel, the one-workgroup-per-candidate scoring kernel, as one template over a variant policy.
// Four translation units instantiate it, each for its own variant and with its own launcher:
//   nmi_kernels.hip          GridPlain    whole aligned 16-byte chunks (or the byte path): the product's main kernel
//   nmi_kernels_gated.hip    GridGated    the same, returning at once unless the few-levels kernels enqueued before it handed the
//                                         search back (plan->use == 0, nmi_fewlevels_kernel.hip)
//   nmi_kernels_rows.hip     GridRows     rows that are not whole aligned chunks (histogram_phase<.., ROWS>)
//   nmi_kernels_stamped.hip  GridStamped  tools only: wall-clock stamps of one candidate of every workgroup at the phase boundaries
// One unit per variant: the kernel sits at its register cap, and when the gated form was first tried as further instantiations
// beside the plain ones their mere presence changed the plain kernel's allocation (not measured again since).
#pragma once
#include "nmi_grid_device.h"

#ifndef NMI_WAVE_SLABS
#define NMI_WAVE_SLABS 1  // 0: equal pixel shares for all wavefronts, as before the slabs (timing comparisons only)
#endif

namespace nmi {

template <bool GATED, bool ROWS, bool STAMPED>
struct GridVariant {
    static constexpr bool gated = GATED, rows = ROWS, stamped = STAMPED;
};
struct GridPlain : GridVariant<false, false, false> {};
struct GridGated : GridVariant<true, false, false> {};
struct GridRows : GridVariant<false, true, false> {};
struct GridStamped : GridVariant<false, false, true> {
    static __device__ uint32_t candidate();  // which candidate of every workgroup is stamped, its k-th (nmi_kernels_stamped.hip)
};

namespace {

// 16-pixel chunks of a pair, histogram_phase's c_end.  An expression at each use, not a value the kernel keeps: held in one local
// variable it reordered the kernel's prologue.
template <class Variant>
__device__ __forceinline__ int grid_chunks(const GridArgs &a)
{
    if constexpr (Variant::rows) return a.height * a.chunks_per_row;
    else return a.npix >> 4;
}

// Stamp K of this workgroup's stamped candidate: a.dbg_stamps[workgroup][8], by the first lane of wavefront 0 (K = 7: of wavefront
// 1).  Nothing unless Variant::stamped.
template <class Variant, int K>
__device__ __forceinline__ void grid_stamp(const GridArgs &a, int tid, bool stamp_on)
{
    if constexpr (Variant::stamped) {
        if (a.dbg_stamps && tid == (K == 7 ? 64 : 0) && stamp_on) a.dbg_stamps[blockIdx.x * 8 + K] = wall_clock64();
    }
}

}  // namespace

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
// GridStamped stamps one candidate of every workgroup -- its k-th, k = GridStamped::candidate(), 0 by default (NMI_OPT_STAMPS,
// NMI_OPT_STAMP_CANDIDATE, tools/grid_stamps.py).  In that unit the wavefronts' pixel shares (slab_cum, nmi_grid_device.h) are a
// device variable that NMI_OPT_WAVE_SHARES overwrites: the calibration runs.
template <class Variant, bool BG, bool SHIFTED, int HIST>
__global__ __launch_bounds__(NMI_BLOCK_THREADS) void nmi_grid_kernel(GridArgs a)
{
    __shared__ Lds lds;
    if constexpr (Variant::gated) {
        if (a.plan->use != 0u) return;
    }
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    bool stamp_on = true;  // inside the loop: the workgroup's k-th candidate only
    int stamp_ordinal = 0;
    if constexpr (Variant::stamped) stamp_ordinal = slot_in_round(blockIdx.x, gridDim.x) + (int)Variant::candidate() * (int)gridDim.x;
    grid_stamp<Variant, 0>(a, tid, stamp_on);
    constexpr bool kOptimistic = HIST == 3;
    constexpr int kFirst = kOptimistic ? 2 : HIST;
    constexpr bool kRows = Variant::rows;  // rows that are not whole aligned chunks (histogram_phase)
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
    grid_stamp<Variant, 1>(a, tid, stamp_on);

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
        if constexpr (Variant::stamped) stamp_on = ordinal == stamp_ordinal;
        grid_stamp<Variant, 7>(a, tid, stamp_on);  // wavefront 1 starts on this candidate's pixels (wavefront 0 may have had the previous one to score)

        if (a.phase_mask & 1) {
            if (a.phase_mask & 8) {  // ablation: only half of the wavefronts take part in the histogram phase
                if (wave < kWaves / 2) histogram_phase<kCountAll, SHIFTED, kFirst, kBlock / 2, true, kRows>(lds, par, a, render, warped, tid, 0, grid_chunks<Variant>(a));
            } else
                histogram_phase<kCountAll, SHIFTED, kFirst, kBlock, true, kRows, kSlabs>(lds, par, a, render, warped, tid, 0, grid_chunks<Variant>(a), ordinal != slot);
        }
        if (table_pending) {
#pragma unroll
            for (int k = 0; k < kLdsTable / kBlock; ++k) lds.table[tid + k * kBlock] = tab[k];
            table_pending = false;
        }
        grid_stamp<Variant, 2>(a, tid, stamp_on);  // this wavefront's share of the pixels done
        if constexpr (Variant::stamped) {
            // ... and every wavefront's, behind the [workgroups][8] block: [workgroups][16]
            if (a.dbg_stamps && lane == 0 && stamp_on) a.dbg_stamps[gridDim.x * 8 + blockIdx.x * 16 + wave] = wall_clock64();
        }
        __syncthreads();  // B1
        grid_stamp<Variant, 3>(a, tid, stamp_on);
        const bool kept = keep_ok && w == kept_w && !(s == 0 && a.plan);
        if (a.phase_mask & 2) {
            if (kKeepWarp && kept) decode_phase<false, true>(lds, par, a, wave, lane);
            else decode_phase<kZero0>(lds, par, a, wave, lane);
        }
        kept_w = w;
        __syncthreads();  // B2
        grid_stamp<Variant, 4>(a, tid, stamp_on);
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
        grid_stamp<Variant, 5>(a, tid, stamp_on);  // score committed (wavefront 0)
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
    grid_stamp<Variant, 6>(a, tid, true);
}

}  // namespace nmi
