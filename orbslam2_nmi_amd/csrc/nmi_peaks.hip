// nmi_peaks.hip -- the K best separated candidates of a rating table (include/nmi_hip.h, "Ranked peaks").
//
// One workgroup of 1024 lanes ranks the whole table: the K rounds are sequential by definition, and a table of up to 65,536 cells
// fits the workgroup's registers.  Lane t owns the cells t + 1024 j, j < CPL (1, 4, 16 or 64 by the table's size), loaded once
// with coalesced loads and kept as score bits; a 64-bit register mask says which of them are out (never qualified, or inside the
// box of an earlier peak).  A round:
//   each lane's best live cell, cached: scanned again only after that cell itself went out
//   the 64-bit key maximum of a wavefront by shuffles, of the 16 wavefronts through the LDS (barrier 1)
//   every lane reads the same winner (lane k of the first wavefront keeps round k's); the lanes together walk the winner's clipped
//   box (at most the product of 2 r + 1) and set the bits of its cells in an LDS copy of the masks (8 KB: 64 bits per lane), which
//   each lane then ORs into its own (barrier 2)
// After the rounds the first wavefront stores the K keys, one lane each, and -- for a caller that polls -- posts the call's sequence
// number behind them.  Nothing else is written to memory and nothing survives the launch: the LDS masks are cleared at its start.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nmi_peaks.h"

namespace nmi {

constexpr int kPeaksThreads = 1024, kPeaksWaves = kPeaksThreads / 64;

__device__ __forceinline__ unsigned long long peaks_wave_max(unsigned long long key)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const unsigned long long other = __shfl_xor(key, off, 64);
        key = other > key ? other : key;
    }
    return key;
}

template <int CPL>
__global__ __launch_bounds__(kPeaksThreads) void nmi_peaks_kernel(PeaksArgs a)
{
    __shared__ uint32_t out_bits[kPeaksThreads * 2];  // bit j of lane t's pair: cell t + 1024 j is inside an earlier peak's box
    __shared__ unsigned long long wave_best[kPeaksWaves];
    const int tid = (int)threadIdx.x;
    const int n = a.cells, K = a.K;
    uint32_t bits[CPL];           // score bits of the lane's cells (-0.0 as 0.0: nmi_key_pack's)
    unsigned long long out = 0;   // bit j: cell j of the lane is out
    float v[CPL];
#pragma unroll
    for (int j = 0; j < CPL; ++j) {  // every load unconditional (past the end: the last cell again), so that all are in flight at once
        const int cell = tid + kPeaksThreads * j;
        v[j] = a.ratings[cell < n ? cell : n - 1];
    }
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
        bits[j] = v[j] == 0.0f ? 0u : __float_as_uint(v[j]);
        if (!(v[j] >= 0.0f) || tid + kPeaksThreads * j >= n) out |= 1ull << j;  // negative, NaN, or no cell
    }
    out_bits[2 * tid] = 0;
    out_bits[2 * tid + 1] = 0;
    __syncthreads();

    int best_j = -1, count = 0;
    uint32_t best_bits = 0;
    unsigned long long mine = 0;  // lane k < K: the key of peak k
    bool scan = true;
    for (int round = 0; round < K; ++round) {
        if (scan) {
            best_j = -1, best_bits = 0;
#pragma unroll
            for (int j = 0; j < CPL; ++j)  // ascending cell index and a strict compare: the lowest index of equal scores
                if (!((out >> j) & 1) && (best_j < 0 || bits[j] > best_bits)) best_bits = bits[j], best_j = j;
            scan = false;
        }
        unsigned long long key = 0;
        if (best_j >= 0) key = ((unsigned long long)best_bits << 32) | (0xFFFFFFFFu - (uint32_t)(tid + kPeaksThreads * best_j));
        key = peaks_wave_max(key);
        if ((tid & 63) == 0) wave_best[tid >> 6] = key;
        __syncthreads();
        unsigned long long win = 0;
#pragma unroll
        for (int w = 0; w < kPeaksWaves; ++w) win = wave_best[w] > win ? wave_best[w] : win;
        if (win == 0) break;  // no qualifying cell is left (the same value in every lane: all leave together)
        if (tid == round) mine = win;
        ++count;
        if (round + 1 == K) break;
        // the winner's box, clipped at the grid's edges (wave-uniform arithmetic)
        uint32_t rem = 0xFFFFFFFFu - (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)win);
        uint32_t lo[6], ext[6], stride[6], box = 1, s = 1;
#pragma unroll
        for (int x = 0; x < 6; ++x) {
            const uint32_t num = (uint32_t)a.num[x], r = (uint32_t)a.radius[x], c = rem % num;
            rem /= num;
            lo[x] = c > r ? c - r : 0;
            const uint32_t hi = c + r < num - 1 ? c + r : num - 1;
            ext[x] = hi - lo[x] + 1;
            box *= ext[x];
            stride[x] = s;
            s *= num;
        }
        for (uint32_t t = (uint32_t)tid; t < box; t += kPeaksThreads) {
            uint32_t q = t, cell = 0;
#pragma unroll
            for (int x = 0; x < 6; ++x) {
                cell += (lo[x] + q % ext[x]) * stride[x];
                q /= ext[x];
            }
            // cell < n <= 65536: lane cell & 1023, its cell number cell >> 10 < 64
            atomicOr(&out_bits[2 * (cell & (kPeaksThreads - 1)) + (cell >> 15)], 1u << ((cell >> 10) & 31));
        }
        __syncthreads();
        out |= (unsigned long long)out_bits[2 * tid] | ((unsigned long long)out_bits[2 * tid + 1] << 32);
        if (best_j >= 0 && ((out >> best_j) & 1)) scan = true;
    }
    if (tid >= 64) return;  // (K <= 64: the keys are the first wavefront's)
    if (tid < K) {
        const unsigned long long key = tid < count ? mine : 0;
        if (a.out) a.out[tid] = key;
        if (a.out_host) a.out_host[tid] = key;
    }
    if (a.post) {  // the keys first, for every lane of the wavefront; then the word the host polls
        __threadfence_system();
        if (tid == 0) __hip_atomic_store(a.post, a.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

hipError_t launch_peaks(const PeaksArgs &a, hipStream_t stream)
{
    if (a.cells < 1 || a.cells > kPeaksMaxCells || a.K < 1 || a.K > kPeaksMaxK || !a.ratings || (!a.out && !a.out_host))
        return hipErrorInvalidValue;
    const dim3 grid(1), block(kPeaksThreads);
    if (a.cells <= kPeaksThreads)
        hipLaunchKernelGGL(nmi_peaks_kernel<1>, grid, block, 0, stream, a);
    else if (a.cells <= 4 * kPeaksThreads)
        hipLaunchKernelGGL(nmi_peaks_kernel<4>, grid, block, 0, stream, a);
    else if (a.cells <= 16 * kPeaksThreads)
        hipLaunchKernelGGL(nmi_peaks_kernel<16>, grid, block, 0, stream, a);
    else
        hipLaunchKernelGGL(nmi_peaks_kernel<64>, grid, block, 0, stream, a);
    return hipGetLastError();
}

}  // namespace nmi
