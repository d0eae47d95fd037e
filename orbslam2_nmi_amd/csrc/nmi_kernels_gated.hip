// nmi_kernels_gated.hip -- nmi_grid_kernel's gated instantiations (GridGated, nmi_grid_kernel.h) and launch_grid_gated: the
// fallback launch behind the few-levels kernels (nmi_fewlevels_kernel.hip), which returns at once unless they handed the search
// back.  A unit of its own: see nmi_grid_kernel.h.
#include "nmi_grid_kernel.h"

namespace nmi {

// 256 bins or the background rule on (the launch is refused otherwise), default histogram variant.
hipError_t launch_grid_gated(const GridArgs &a, int workgroups, bool use_bg, hipStream_t stream)
{
    if (a.hist_variant != 3 || !a.plan || (a.shift != 0 && !use_bg)) return hipErrorInvalidValue;
    with_bg_shifted(use_bg, a.shift != 0, [&](auto bg, auto shifted) {
        if constexpr (bg.value || !shifted.value)
            hipLaunchKernelGGL((nmi_grid_kernel<GridGated, bg.value, shifted.value, 3>), dim3(workgroups), dim3(kBlock), 0, stream, a);
    });
    return hipGetLastError();
}

}  // namespace nmi
