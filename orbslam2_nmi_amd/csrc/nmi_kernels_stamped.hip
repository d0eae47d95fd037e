// nmi_kernels_stamped.hip -- nmi_grid_kernel once more, as nmi_grid_kernel_stamped + launch_grid_stamped: the same code with
// wall-clock stamps at the phase boundaries of one candidate of every workgroup (NMI_OPT_STAMPS, NMI_OPT_STAMP_CANDIDATE;
// tools/grid_stamps.py), and with the wavefronts' pixel shares in a device variable that NMI_OPT_WAVE_SHARES overwrites.
// A translation unit of its own so that the product's kernel is not touched by the instrumentation.
#define NMI_GRID_KERNEL_STAMPED 1
#define NMI_SLAB_SHARES_QUALIFIER __device__
#include "nmi_kernels.hip"
