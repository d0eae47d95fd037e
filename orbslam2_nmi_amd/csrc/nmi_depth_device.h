// nmi_depth_device.h -- the depth shade (include/nmi_hip.h, "Depth maps"): what a depth render shows of the winner of a pixel.
// Every depth shader -- the point renderer's resolve kernels (nmi_producers.hip), the mesh renderer's tile kernels
// (nmi_mesh.hip), nmi_depth_shade_apply (nmi_depth.hip) -- calls depth_shade() below and nothing else: the output is a pure
// function of the winner's 24 depth bits.  tests/helpers/depth_np.py restates it in numpy.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nmi_kernels.h"   // struct DepthShade

namespace nmi {

// The rule, in fp32, every operation rounded on its own (the build forbids contraction; both divisions are IEEE divisions):
//   u   = (float)(2^24 - 1 - d) / (2^24 - 1)         1 - zw; the numerator is exact
//   den = near + u (far - near)
//   z   = (near far) / den                           eye-space Z of window depth zw under nmi_render_mvp's projection
//   v   = clamp((uint32)(z scale + 0.5), 1, 65535)   raw 16-bit depth; 0 is kept for "nothing there"
//   grey = NMI_TONE_WINDOW(lo, hi) of v              v <= lo: 0, v >= hi: 255, else ((v - lo) 255 + ((hi - lo) >> 1)) / (hi - lo)
// (the clamp is taken on the float, before the conversion: the same value for every float, and no conversion out of range)
//
// The window's integer division is taken without the 25-instruction integer divide (the resolve kernels are bound by instruction
// issue once they shade): with c = clamp(v, lo, hi) the rule is n / span for n = (c - lo) 255 + (span >> 1), span = hi - lo, at
// both ends too (n / span = 0 at c = lo, 255 at c = hi).  n < 2^24 is exact in fp32 and the quotient is below 256, so
// t = (float)n * (1 / (float)span) is within 256 * 2^-22 of it: (uint32)t is the quotient or one beside it, and the remainder
// says which.  Integers decide; no rounding of t reaches the result.
__device__ __forceinline__ void depth_shade(const DepthShade &sh, uint32_t d, uint32_t &v, uint32_t &grey)
{
    const float u = (float)(16777215u - d) / 16777215.0f;
    const float den = sh.near_plane + u * (sh.far_plane - sh.near_plane);
    const float z = (sh.near_plane * sh.far_plane) / den;
    v = (uint32_t)fminf(fmaxf(z * sh.scale + 0.5f, 1.0f), 65535.0f);
    const uint32_t span = sh.hi - sh.lo;
    const float inv_span = 1.0f / (float)span;      // (the same for every pixel: the compiler keeps it out of the loops)
    const uint32_t n = __umul24(min(max(v, sh.lo), sh.hi) - sh.lo, 255u) + (span >> 1);
    uint32_t q = (uint32_t)((float)n * inv_span);
    const int32_t r = (int32_t)(n - __umul24(q, span));
    grey = q + (r >= (int32_t)span ? 1u : 0u) - (r < 0 ? 1u : 0u);
}

// An uncovered pixel: v = 0, grey = 255 (the background every renderer clears to).
constexpr uint32_t kDepthNothing = 0u, kDepthBackground = 255u;

}  // namespace nmi
