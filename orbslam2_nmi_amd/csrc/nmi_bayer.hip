// nmi_bayer.hip -- 8-bit Bayer mosaics to the dense grey frame the warps read (nmi_gray_frame and nmi_reduce_frame under an
// NMI_FRAME_BAYER_* format, include/nmi_hip.h): each mosaic site demosaiced bilinearly and weighted to grey with one rounding
// (nmi_bayer_device.h), then, at a factor F = 2, 3 or 4, the rounded box average of each F x F block (nmi_reduce_device.h).  A
// mosaic is one byte per pixel, a third of an RGB frame's; a site reads its 3 x 3 neighbourhood, so a lane's four output
// pixels share one (F + 2) x (4 F + 2) window.  No LDS: neighbouring lanes and rows meet in the caches.  A distorted mosaic is
// demosaiced here first and undistorted from the grey frame (nmi_intake.h): a tap that demosaics costs nine loads.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nmi_hip.h"
#include "nmi_bayer_device.h"
#include "nmi_color.h"
#include "nmi_reduce_device.h"

namespace nmi {

namespace {

constexpr int kBayerQuads = 64;  // lanes per block row: 4 x 64 = 256 output pixels; 4 block rows (the conversion kernel's shape)

}  // namespace

// A lane makes 4 adjacent pixels of one output row from the mosaic bytes (sx - 1 .., sy - 1 ..), sx = 4 F q, sy = F y: F + 2
// rows of 4 F + 2.  Inside the frame the window is read as it lies: with vec_in (every source row starts on a 4-byte boundary,
// base and pitch) its middle 4 F bytes come as F dwords and the two ends as bytes, otherwise all as bytes.  A window that
// reaches over the frame's first or last column or row -- the last quad of a row among them, whatever the width -- is read
// through reflected coordinates (bayer_reflect); nothing outside the factor * width x factor * height pixels is read.  vec_out:
// width % 4 == 0 and gray 4-byte aligned, one dword store; otherwise byte stores.  phase: nmi_bayer_device.h.
template <int F>
__global__ __launch_bounds__(256) void nmi_bayer_kernel(const uint8_t *__restrict__ src, size_t pitch, int phase, uint8_t *__restrict__ gray,
                                                        int width, int height, int vec_in, int vec_out)
{
    constexpr int WC = 4 * F + 2, WR = F + 2;
    const int q = blockIdx.x * kBayerQuads + (int)threadIdx.x;
    const int y = blockIdx.y * 4 + (int)threadIdx.y;
    const int x0 = q * 4;
    if (x0 >= width || y >= height) return;
    const int n = min(4, width - x0);
    const int fw = width * F, fh = height * F, sx = x0 * F, sy = y * F;
    uint32_t win[WR][WC];  // win[r][i] = the mosaic byte at (sx - 1 + i, sy - 1 + r)
    if (sx >= 1 && sx + 4 * F < fw && sy >= 1 && sy + F < fh) {
#pragma unroll
        for (int r = 0; r < WR; ++r) {
            const uint8_t *row = src + (size_t)(sy - 1 + r) * pitch + sx;
            win[r][0] = row[-1];
            win[r][WC - 1] = row[4 * F];
            if (vec_in) {
                uint32_t w[F];
                __builtin_memcpy(w, __builtin_assume_aligned(row, 4), 4 * F);
#pragma unroll
                for (int i = 0; i < 4 * F; ++i) win[r][1 + i] = (w[i / 4] >> (8 * (i % 4))) & 255u;
            } else {
#pragma unroll
                for (int i = 0; i < 4 * F; ++i) win[r][1 + i] = row[i];
            }
        }
    } else {
        int xi[WC];  // (columns past the reflected one belong to pixels beyond the row's end, which are not stored: any byte of the row)
#pragma unroll
        for (int i = 0; i < WC; ++i) xi[i] = min(max(bayer_reflect(sx - 1 + i, fw), 0), fw - 1);
#pragma unroll
        for (int r = 0; r < WR; ++r) {
            const uint8_t *row = src + (size_t)bayer_reflect(sy - 1 + r, fh) * pitch;
#pragma unroll
            for (int i = 0; i < WC; ++i) win[r][i] = row[xi[i]];
        }
    }
    const int pa = phase & 1, pb = phase >> 1;
    uint32_t packed = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        uint32_t s = 0;
#pragma unroll
        for (int r = 0; r < F; ++r) {
            const int b = ((sy + r) ^ pb) & 1;
#pragma unroll
            for (int j = 0; j < F; ++j) {
                const int i = k * F + j + 1;  // the site's window column; sx is even, so its column parity is (i - 1) & 1
                const uint32_t hs = win[r + 1][i - 1] + win[r + 1][i + 1], vs = win[r][i] + win[r + 2][i];
                const uint32_t ds = win[r][i - 1] + win[r][i + 1] + win[r + 2][i - 1] + win[r + 2][i + 1];
                s += bayer_gray(win[r + 1][i], hs, vs, ds, ((i - 1) ^ pa) & 1, b);
            }
        }
        packed |= reduce_round<F>(s) << (8 * k);
    }
    const size_t o = (size_t)y * width + x0;
    if (vec_out) {  // (width % 4 == 0: the quad lies wholly inside the row)
        *reinterpret_cast<uint32_t *>(gray + o) = packed;
    } else {
        for (int k = 0; k < n; ++k) gray[o + k] = (uint8_t)(packed >> (8 * k));
    }
}

namespace {

template <int F>
void bayer_launch(const uint8_t *src, size_t pitch, int phase, uint8_t *gray, int width, int height, hipStream_t stream)
{
    const int quads = (width + 3) / 4;
    const dim3 grid((quads + kBayerQuads - 1) / kBayerQuads, (height + 3) / 4), block(kBayerQuads, 4);
    const int vec_in = ((uintptr_t)src % 4) == 0 && (pitch % 4) == 0;
    const int vec_out = (width % 4) == 0 && ((uintptr_t)gray % 4) == 0;
    hipLaunchKernelGGL((nmi_bayer_kernel<F>), grid, block, 0, stream, src, pitch, phase, gray, width, height, vec_in, vec_out);
}

}  // namespace

hipError_t launch_bayer(const uint8_t *src, int format, int64_t pitch, int factor, uint8_t *gray, int width, int height, hipStream_t stream)
{
    if (!frame_is_bayer(format) || (int64_t)factor * width < 2 || (int64_t)factor * height < 2) return hipErrorInvalidValue;
    const int phase = format - NMI_FRAME_BAYER_RGGB;  // bit 0: the red sites' column parity, bit 1: their row parity
    const size_t pb = (size_t)pitch;
    switch (factor) {
    case 1: bayer_launch<1>(src, pb, phase, gray, width, height, stream); break;
    case 2: bayer_launch<2>(src, pb, phase, gray, width, height, stream); break;
    case 3: bayer_launch<3>(src, pb, phase, gray, width, height, stream); break;
    case 4: bayer_launch<4>(src, pb, phase, gray, width, height, stream); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace nmi
