// nmi_kernels_stamped.hip -- tools only: nmi_grid_kernel<GridStamped, true, false, 3> (nmi_grid_kernel.h) and launch_grid_stamped:
// the product's main kernel with wall-clock stamps at the phase boundaries of one candidate of every workgroup (NMI_OPT_STAMPS,
// NMI_OPT_STAMP_CANDIDATE; tools/grid_stamps.py), and with the wavefronts' pixel shares in a device variable that
// NMI_OPT_WAVE_SHARES overwrites.  A unit of its own so that the product's kernel is not touched by the instrumentation.
#define NMI_SLAB_SHARES_QUALIFIER __device__  // slab_cum (nmi_grid_device.h): writable in this unit
#include "nmi_grid_kernel.h"

namespace nmi {

namespace {
__device__ uint32_t stamp_candidate = 0;  // which candidate of every workgroup is stamped (its k-th)
}
__device__ __forceinline__ uint32_t GridStamped::candidate() { return stamp_candidate; }

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

// 256 bins, background rule on, default histogram variant
hipError_t launch_grid_stamped(const GridArgs &a, int workgroups, hipStream_t stream)
{
    if (a.hist_variant != 3 || a.shift != 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL((nmi_grid_kernel<GridStamped, true, false, 3>), dim3(workgroups), dim3(kBlock), 0, stream, a);
    return hipGetLastError();
}

}  // namespace nmi
