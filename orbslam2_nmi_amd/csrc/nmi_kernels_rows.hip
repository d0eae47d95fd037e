// nmi_kernels_rows.hip -- nmi_grid_kernel's instantiations for frames whose rows are not whole aligned 16-byte chunks (GridRows,
// nmi_grid_kernel.h: width % 16 != 0 -- KITTI's 1241 x 376 -- or stacks that are not 16-byte aligned) and launch_grid_rows.  Same
// kernel; the histogram phase addresses chunks per row with unaligned 16-byte loads and adds each row's last width % 16 pixels
// one by one (histogram_phase<..., ROWS = true>, nmi_grid_device.h).  A unit of its own: see nmi_grid_kernel.h.
#include "nmi_grid_kernel.h"

namespace nmi {

hipError_t launch_grid_rows(const GridArgs &a, int workgroups, bool use_bg, hipStream_t stream)
{
    if (a.width < 32 || (a.hist_variant != 1 && a.hist_variant != 3)) return hipErrorInvalidValue;
    const dim3 grid(workgroups), block(kBlock);
    const bool exact_only = a.hist_variant == 1 || (!use_bg && a.shift != 0);  // (as launch_grid: BG off below 256 bins has no optimistic path)
    with_bg_shifted(use_bg, a.shift != 0, [&](auto bg, auto shifted) {
        if (exact_only) hipLaunchKernelGGL((nmi_grid_kernel<GridRows, bg.value, shifted.value, 1>), grid, block, 0, stream, a);
        else if constexpr (bg.value || !shifted.value) hipLaunchKernelGGL((nmi_grid_kernel<GridRows, bg.value, shifted.value, 3>), grid, block, 0, stream, a);
    });
    return hipGetLastError();
}

}  // namespace nmi
