// nmi_mesh_color.h -- launch declaration of the vertex-coloured mesh renderer (nmi_mesh_color.hip: nmi_mesh.hip built with
// NMI_MESH_COLOR).  Work area, limits and the warp workgroups that ride along are launch_render_mesh's (nmi_kernels.h); `red` is
// float [3T], one colour per corner in the order of xyz, and there is no texture.
#pragma once
#include "nmi_kernels.h"

namespace nmi {

hipError_t launch_render_mesh_colored(const float *xyz, const float *red, long long ntri, const float *mvps /*[S][16]*/, int S, const MeshWork &w,
                                      int layout_views /* views the work area was allocated for (>= S) */, int bin_cap_limit,
                                      unsigned long long clip_cap_limit, uint8_t *out, int width, int height, hipStream_t stream,
                                      const uint8_t *warp_frame = nullptr, const float *warp_coeffs = nullptr, uint8_t *warp_out = nullptr, int Wn = 0,
                                      uint8_t *cover = nullptr);

}  // namespace nmi
