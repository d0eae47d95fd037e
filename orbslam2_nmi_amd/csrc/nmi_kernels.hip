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
// same launch.  Histogramming is integer scatter work: no MFMA.
//
// The kernel is the template of nmi_grid_kernel.h; here are its plain instantiations (GridPlain), the term-table kernel and
// launch_grid, which sends the other forms to their units' launchers (nmi_kernels_rows / _stamped / _ablate.hip).
#include "nmi_grid_kernel.h"

namespace nmi {

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
    with_bg_shifted(use_bg, a.shift != 0, [&](auto bg, auto shifted) {
        hipLaunchKernelGGL((nmi_grid_kernel<GridPlain, bg.value, shifted.value, HIST>), grid, block, 0, stream, a);
    });
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
#ifdef NMI_BUILD_ABLATIONS  // experiments kept for tools/ablate.py; not part of the shipped library (profiles/NOTES.md)
    case 0: launch_hist<0>(a, grid, block, use_bg, stream); break;
    case 2: launch_hist<2>(a, grid, block, use_bg, stream); break;
    case 4:
        // pipelined kernel (experimental).  It has no debug exports and needs BG on.
        if (use_bg && !a.dbg_joint && !a.dbg_h1 && !a.dbg_h2 && !a.dbg_sums)
            return launch_grid_pipelined(a, workgroups, stream);
        else if (use_bg)
            launch_hist<3>(a, grid, block, use_bg, stream);
        else
            launch_hist<1>(a, grid, block, use_bg, stream);
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

}  // namespace nmi
