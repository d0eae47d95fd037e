// nmi_kernels_ablate.hip -- the ablation build's pipelined form of nmi_grid_kernel (NMI_OPT_HIST_VARIANT = 4) and its launcher,
// launch_grid_pipelined, which launch_grid calls.  Empty unless NMI_BUILD_ABLATIONS (python -m orbslam2_nmi_amd.build --ablations,
// tools/ablate.py): not part of the shipped library (profiles/NOTES.md).
#ifdef NMI_BUILD_ABLATIONS
#include "nmi_grid_device.h"

namespace nmi {

// ---------------------------------------------------------------------------------------------------------
// Pipelined ("wavefront-specialised") form of the same computation (NMI_OPT_HIST_VARIANT = 4, experimental).
// Exact, covered by the parity tests, but measured SLOWER than the sequential kernel on MI355X (114 vs 95 us per 729
// candidates): the decode wavefronts take issue slots from the histogram wavefronts, 8 histogram wavefronts add
// pixels 22 % slower than 16, and the drain is a third serial step.  Kept as an ablation; see profiles/NOTES.md.
//
// The histogram phase is bound by the LDS atomic unit, the decode arithmetic by VALU issue and latency; run one
// after the other (nmi_grid_kernel) a CU leaves each unit idle in turn.  Here the 16 wavefronts split into
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
    clear_lds(lds, tid);
    for (int c = tid; c < kLdsTable; c += kBlock) lds.table[c] = a.table[c <= a.npix ? c : 0];
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

// BG on, no debug exports (launch_grid sends every other launch of the variant to the sequential kernel).
hipError_t launch_grid_pipelined(const GridArgs &a, int workgroups, hipStream_t stream)
{
    hipLaunchKernelGGL(a.shift != 0 ? nmi_grid_kernel_ws<true> : nmi_grid_kernel_ws<false>, dim3(workgroups), dim3(kBlock), 0, stream, a);
    return hipGetLastError();
}

}  // namespace nmi
#endif  // NMI_BUILD_ABLATIONS
