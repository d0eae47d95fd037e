// nmi_pix_kernel.hip -- the scoring path for MID-SIZE grids (33 ... 128 candidates on 256 compute units): P workgroups per
// candidate, each adding a PIXEL RANGE of the pair into a whole packed joint histogram of its own.
//
// Why: the live search seeds its grid from the drift and collapses every axis whose step falls under the minimum
// (src/Tracking.cc:2014-2043, Thirdparty/Localization/nmiSearchKernel.cpp:124-141): 27 / 81 / 243-candidate grids are its
// typical levels, and a rank's share of a sharded 729-candidate grid is 91.  nmi_grid_kernel gives a candidate to one
// workgroup = one CU: 81 candidates take as long as 256 (35 us) with two thirds of the chip idle.  The row split of
// nmi_split_kernel.hip does not help there: a part issues one LDS atomic instruction per 64 pixels of the WHOLE pair
// however few of its lanes own them, and the time of nmi_grid_kernel's histogram phase is its LDS atomic instructions.
//
// How: workgroup (candidate p, range q) runs nmi_grid_kernel's own histogram phase (NMI.cu:79-87; nmi_grid_device.h:
// packed 16-bit counters, 129 KiB of LDS, one non-returning atomic per pixel, flat regions folded) over chunks
// of its own.  Range 0 is the candidate's OWNER; ranges 1 .. P-1 are HELPERS: a helper writes the 16-byte units of its packed
// histogram that hold a count (+ its flat-region side counters) to its block in memory with write-through stores, every wave
// drains its stores, and after the workgroup's barrier the launch's tag goes out with the masks that say which units came
// (MI355X_MICROARCH.md "Valid forms", first row of the table: sc1 stores, drained, signalled after the barrier; the owner's
// waves poll with sc1 loads and read every byte with 16-byte sc1 loads).  The owner adds the helpers' words to its own LDS
// words -- packed fields add like the counters they are -- and from there on is nmi_grid_kernel:
// decode_phase (ComputeEntropyKernel + AddvectorParwiseMidKernel, NMI.cu:230-287), the wrap detector, final_phase
// (AddVectorPairwiseKernel, NMI.cu:290-363), rating store, arg-max, completion.  Results are bit-identical.
//   * Counter wraps: a wrapped 16-bit field always LOSES weight, in a helper, in the owner or in the merge, so the sum of all
//     decoded counters still equals W*H iff nothing wrapped; a candidate that fails is redone by its owner alone on the exact
//     path (exact_candidate), as in nmi_grid_kernel, and counted in timeouts[kPixHealCountTest] (nmi_pix_heal_counts:
//     count_test).  A unit, side counter or mask read stale makes the total fall short in the same way: on content that cannot
//     wrap a field, that counter is how a bad hand-off shows, for the bits come out right either way.
//   * Liveness: helpers never wait, and the owner's wait is bounded: should a helper's flag not arrive within 2 ms
//     (kPixTimeoutTicks), the owner scores the candidate alone on the exact path and counts the event in
//     timeouts[kPixHealTimeouts] (nmi_pix_heal_counts: timeouts) and in timeouts[kPixHealed] (nmi_pix_status: healed).  That
//     bounded wait and the in-launch heal are the guarantee -- the launch always completes and heals itself, the host has
//     nothing to redo -- which is why this form may also be used by calls that only enqueue.  The helpers are the FIRST
//     total * (P - 1) workgroups of the launch, so they usually run before or beside their owners; but each XCD dispatches
//     on its own, and an owner may start before a lower-numbered helper whose CUs are held by other work (another stream's
//     launch, say).  Such a stall costs up to 2 ms and shows as a rising timeout count, never as a wrong result.
//   * Tags: 0x80000000 | (host epoch + replay word) mod 2^31; the replay word lives in device memory for launches that are
//     replayed from a captured graph with frozen arguments (bumped by the graph's first node), absent otherwise.
//
// Shared with nmi_masked_pix_kernel.hip and nmi_covered_pix_kernel.hip, in nmi_pix_device.h: which workgroup scores what
// (pix_unit), the dealing and the pieces' addressing (make_deal, Pieces), the counter clear, the hand-off (pix_publish,
// pix_collect: here with the side counters beside the units), the merged decode (decode_merged with TableTerms) and the
// launchers' dispatch (pix_launch).  This file keeps the kernel's sequence of those steps, its stamps and its own heal.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nmi_pix_device.h"

namespace nmi {

size_t pix_block_bytes(int candidates, int pix_parts) { return (size_t)candidates * (size_t)(pix_parts - 1) * kPixBlockBytes; }

template <bool ZERO0, bool SHIFTED>
__global__ __launch_bounds__(NMI_BLOCK_THREADS) void nmi_pix_kernel(GridArgs a, int P, DealArgs dealing, const uint32_t *replay, uint32_t *timeouts)
{
    __shared__ Lds lds;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    auto stamp = [&](int k) {  // tools/pix_stamps.py: where a workgroup's time goes (100 MHz clock)
        if (a.dbg_stamps && tid == 0) a.dbg_stamps[blockIdx.x * 8 + k] = wall_clock64();
    };
    stamp(0);

    const PixUnit u = pix_unit(a, P, dealing, replay);
    const int q = u.q, p = u.p, w = u.w, s = u.s;
    const bool owner = q == 0;
    const uint8_t *render = a.render_stack + (size_t)s * a.npix;
    const uint8_t *warped = a.warp_stack + (size_t)w * a.npix;

    if (blockIdx.x == 0 && tid == 0 && a.reset_key) *a.reset_key = 0ull;  // next launch's slot; idle during this one
    float tab[kLdsTable / kBlock];
    if (owner) {
#pragma unroll
        for (int k = 0; k < kLdsTable / kBlock; ++k) {
            const int c = tid + k * kBlock;
            tab[k] = a.table[c <= a.npix ? c : 0];
        }
    }
    clear_counters(lds, tid);
    // This workgroup's pixels (frames of at least 32 pixels of width).  The owner's share is the larger one: its
    // helpers' counters need a few microseconds to reach it, which it spends adding pixels.
    const Deal deal = make_deal(dealing, P, q);
    __syncthreads();
    stamp(1);
    histogram_dealt<SHIFTED>(lds, a, render, warped, wave, lane, deal);

    if (!owner) {
        __syncthreads();
        stamp(2);
        pix_publish<true>(lds, a, u, wave, lane);
        stamp(3);
        return;
    }

    // ---- owner ----
#pragma unroll
    for (int k = 0; k < kLdsTable / kBlock; ++k) lds.table[tid + k * kBlock] = tab[k];
    stamp(2);
    u32x4 acc[kUnitsPerLane];
    pix_collect<true>(lds, u, P, wave, lane, acc);
    __syncthreads();  // B1: every wavefront's pixels are in the counters, every helper's side counters in the list
    stamp(3);
    unsigned long long prev_key = 0;
    bool alone = lds.fallback != 0;  // some wave gave up on a helper (workgroup-uniform)
    if (!alone) {
        decode_merged<ZERO0>(lds, TableTerms{a.table, (uint32_t)a.npix, a.dbg_joint}, wave, lane, acc);
        __syncthreads();
        stamp(5);
        alone = lds.total[0] != (uint32_t)a.npix;  // some 16-bit field wrapped (workgroup-uniform, rare)
        if (!alone && wave == 0) final_phase_owner(lds, a, lane, p, w, s, prev_key);
    } else if (tid == 0 && timeouts) {
        pix_count_heal(timeouts, true, false);  // a wait was given up
    }
    if (alone) {
        // cold: this candidate once more, by this workgroup alone, on the exact path
        if (tid == 0 && timeouts && lds.fallback == 0) pix_count_heal(timeouts, false, false);  // the count test failed
        __syncthreads();
        clear_counters(lds, tid);
        __syncthreads();
        exact_candidate<SHIFTED, !ZERO0>(lds, a, tid, p, prev_key);
    }
    stamp(6);
    if (wave == 0) finish_search(a, lane, prev_key, (uint32_t)u.total);
    stamp(7);
}

// One launch of total * pix_parts workgroups.  Needs width >= 32 (rows need not be whole aligned chunks), 256 bins or the
// background rule on, and a.blocks of pix_block_bytes(total, pix_parts), zero when allocated (pix_launch_ok).  A candidate
// that wraps a counter or times out is redone by exact_candidate with ROWS = false: the byte path when !a.vec_ok.  owner_share: the fraction of the pair's pixels the
// owner adds itself (1 / pix_parts: equal shares).
hipError_t launch_pix(const GridArgs &a, int pix_parts, double owner_share, bool use_bg, const uint32_t *replay, uint32_t *timeouts, hipStream_t stream)
{
    if (!pix_launch_ok(a, pix_parts, use_bg)) return hipErrorInvalidValue;
    return pix_launch(a, pix_parts, owner_share, use_bg, [&](auto zero0, auto shifted, dim3 grid, const DealArgs &g) {
        hipLaunchKernelGGL((nmi_pix_kernel<decltype(zero0)::value, decltype(shifted)::value>), grid, dim3(kBlock), 0, stream, a, pix_parts, g, replay, timeouts);
    });
}

}  // namespace nmi
