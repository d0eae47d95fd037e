// nmi_refine.hip -- sub-cell offset, interpolated score and Hessian of K peaks of a rating table (include/nmi_hip.h, "Refined
// peaks").  The arithmetic is nmi_refine_rule.h's, shared with the host twin; this file is the gather around it.
//
// One launch of K workgroups of one wavefront: a record is one wavefront's work.
//   gather   lane t loads sample t, and lanes 0 .. 8 sample 64 + t as well: at most two loads a lane, all unconditional (a sample
//            that would leave the grid is the centre again), so all 73 are in flight at once after the one dependent load of the key
//   solve    the samples go through the LDS (292 bytes) to one lane, which runs refine_rule: about 200 dependent flops on at most
//            6 x 6, nothing a second lane could help with
//   store    the record goes through the LDS too, and lanes 0 .. 37 store one word each (to the device array, to the mapped host
//            array, or both); then, for a caller that polls, lane 0 posts the call's sequence number to the record's own word
// How the samples reach the solve: through the LDS, not by v_readlane or DPP.  gfx950 has no scalar float unit, so a sample taken
// with v_readlane would have to go back into a vector register before its first subtraction: two instructions a sample against
// one ds_read, and the sample's number would have to be a constant of the instruction, where the LDS takes the rule's own
// indices (f[13 + 4 p + q]) as they are.  DPP moves between neighbouring lanes, which is no help to a 73-to-1 funnel.  The cost is
// one barrier of a single wavefront.
// An empty record (key 0, or an index that is no cell) reads nothing from the table.  No atomics but the release store of the
// posted word; nothing survives the launch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nmi_refine.h"

namespace nmi {

constexpr int kRefineThreads = 64;

__global__ __launch_bounds__(kRefineThreads) void nmi_refine_kernel(RefineArgs a)
{
    __shared__ float samples[kRefineSamples];
    __shared__ nmi_refined_peak record;
    const int lane = (int)threadIdx.x, k = (int)blockIdx.x;
    const unsigned long long key = a.keys ? a.keys[k] : a.host_keys[k];
    const uint32_t centre = 0xFFFFFFFFu - (uint32_t)key;
    uint32_t word = lane == 9 ? NMI_REFINE_EMPTY : 0u;  // the empty record: flags are word 9
    if (key != 0 && centre < a.cells) {                 // (the same in every lane)
        int32_t c[6];
        uint32_t stride[6];
        refine_coordinates(centre, a.num, c, stride);
        const int second = lane + kRefineThreads;
        const uint32_t cell0 = refine_sample_cell(lane, centre, c, a.num, stride);
        const uint32_t cell1 = second < kRefineSamples ? refine_sample_cell(second, centre, c, a.num, stride) : centre;
        const float v0 = a.ratings[cell0], v1 = a.ratings[cell1];
        samples[lane] = v0;
        if (second < kRefineSamples) samples[second] = v1;
        __syncthreads();
        if (lane == 0) refine_rule(samples, c, a.num, key, &record);
        __syncthreads();
        if (lane < kRefineWords) word = reinterpret_cast<const uint32_t *>(&record)[lane];
    }
    if (lane < kRefineWords) {
        if (a.out) reinterpret_cast<uint32_t *>(a.out + k)[lane] = word;
        if (a.out_host) reinterpret_cast<uint32_t *>(a.out_host + k)[lane] = word;
    }
    if (a.post) {  // the record first, for every lane of the wavefront; then the word the host polls
        __threadfence_system();
        if (lane == 0) __hip_atomic_store(a.post + k, a.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

hipError_t launch_refine(const RefineArgs &a, hipStream_t stream)
{
    if (a.cells < 1 || a.K < 1 || a.K > kRefineMaxK || !a.ratings || (!a.out && !a.out_host)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(nmi_refine_kernel, dim3((unsigned)a.K), dim3(kRefineThreads), 0, stream, a);
    return hipGetLastError();
}

}  // namespace nmi
