// nmi_unpack.hip -- the deep raw formats to their dense GRAY16 container (include/nmi_hip.h "Deep frames"; nmi_unpack.h):
// big-endian words, PFNC Mono10p / Mono12p, CSI-2 RAW10 / RAW12, and 16-bit Bayer mosaics demosaiced to grey by the 8-bit
// mosaics' rule (nmi_bayer_device.h).  Every deep kernel (nmi_tone.hip, nmi_clahe.hip) reads the container, so a format is known
// here and nowhere else.  Pure streaming: a lane takes one run of 8 output pixels -- 10, 12 or 16 source bytes -- and writes it
// with one 16-byte store; consecutive lanes take consecutive runs of a row.  No LDS; a mosaic's 3 x 10 windows meet in the
// caches, as nmi_bayer.hip's do.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nmi_hip.h"
#include "nmi_bayer_device.h"
#include "nmi_color.h"
#include "nmi_unpack.h"

namespace nmi {

namespace {

constexpr int kUnpackLanes = 64;  // lanes per block row: 64 runs = 512 output pixels; 4 block rows

enum Layout { kBigEndian, kMono10p, kMono12p, kRaw10, kRaw12 };

template <int L> constexpr int run_bytes() { return L == kBigEndian ? 16 : (L == kMono10p || L == kRaw10) ? 10 : 12; }

// The run's 8 container pixels, two per word (the even one low), from its bytes as little-endian words (those past the run's
// bytes are 0 and give pixels that are not stored).
template <int L> __device__ __forceinline__ void decode_run(const uint32_t (&w)[4], uint32_t (&o)[4])
{
    if constexpr (L == kBigEndian) {
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] = ((w[i] & 0x00FF00FFu) << 8) | ((w[i] >> 8) & 0x00FF00FFu);
    } else if constexpr (L == kMono10p || L == kRaw10) {
        // two groups of 4 pixels in 5 bytes, each as one 40-bit value
        const uint64_t v[2] = {w[0] | ((uint64_t)(w[1] & 0xFFu) << 32), (w[1] >> 8) | ((uint64_t)(w[2] & 0xFFFFu) << 24)};
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            uint32_t u[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if constexpr (L == kMono10p)
                    u[i] = (uint32_t)(v[g] >> (10 * i)) & 0x3FFu;
                else
                    u[i] = (((uint32_t)(v[g] >> (8 * i)) & 0xFFu) << 2) | ((uint32_t)(v[g] >> (32 + 2 * i)) & 3u);
            }
            o[2 * g] = u[0] | (u[1] << 16);
            o[2 * g + 1] = u[2] | (u[3] << 16);
        }
    } else {
        // four groups of 2 pixels in 3 bytes, each as one 24-bit value
        const uint32_t t[4] = {w[0] & 0xFFFFFFu, (w[0] >> 24) | ((w[1] & 0xFFFFu) << 8), (w[1] >> 16) | ((w[2] & 0xFFu) << 16), w[2] >> 8};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if constexpr (L == kMono12p)
                o[j] = (t[j] & 0xFFFu) | ((t[j] >> 12) << 16);
            else
                o[j] = (((t[j] & 0xFFu) << 4) | ((t[j] >> 16) & 15u)) | (((((t[j] >> 8) & 0xFFu) << 4) | (t[j] >> 20)) << 16);
        }
    }
}

// The first n of the run's pixels to dst.  vec 2: one 16-byte store (the container row allows it: base on 16 bytes, width % 8
// == 0, so n == 8); vec 1: 8-byte stores (base on 8 bytes, width % 4 == 0, so n is 4 or 8); vec 0: pixel by pixel.
__device__ __forceinline__ void store_run(uint16_t *dst, const uint32_t (&o)[4], int n, int vec)
{
    if (vec == 2) {
        *reinterpret_cast<uint4 *>(dst) = make_uint4(o[0], o[1], o[2], o[3]);
    } else if (vec == 1) {
        *reinterpret_cast<uint2 *>(dst) = make_uint2(o[0], o[1]);
        if (n == 8) *reinterpret_cast<uint2 *>(dst + 4) = make_uint2(o[2], o[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (k < n) dst[k] = (uint16_t)(o[k / 2] >> (16 * (k & 1)));
    }
}

}  // namespace

// A byte layout.  A lane's run starts run_bytes() * its index into the row: any byte address for the packed layouts (the row's
// base and pitch are free), so it is loaded with alignment 1, never through an aligned vector type.  A whole run lies inside
// the row's bytes; the row's tail run is read byte by byte up to the row's last byte, and no further.
template <int L>
__global__ __launch_bounds__(256) void nmi_unpack_kernel(const uint8_t *__restrict__ src, size_t pitch, uint16_t *__restrict__ gray16, int width,
                                                         int height, int vec)
{
    constexpr int NB = run_bytes<L>();
    const int run = blockIdx.x * kUnpackLanes + (int)threadIdx.x;
    const int y = blockIdx.y * 4 + (int)threadIdx.y;
    const int x0 = run * 8;
    if (x0 >= width || y >= height) return;
    const int n = min(8, width - x0);
    const uint8_t *p = src + (size_t)y * pitch + (size_t)run * NB;
    uint32_t w[4] = {0u, 0u, 0u, 0u}, o[4];
    if (n == 8) {
        __builtin_memcpy(w, p, NB);
    } else {
        const int nb = n * NB / 8;  // (whole groups: exact)
#pragma unroll
        for (int i = 0; i < NB; ++i)
            if (i < nb) w[i / 4] |= (uint32_t)p[i] << (8 * (i % 4));
    }
    decode_run<L>(w, o);
    store_run(gray16 + (size_t)y * width + x0, o, n, vec);
}

// A 16-bit mosaic: the run's 8 sites from the 3 x 10 sites around them, win[r][i] = the site at (x0 - 1 + i, y - 1 + r).  Inside
// the frame the window is read as it lies (its middle 8 sites as 16 bytes on the sites' 2-byte alignment); a window that reaches
// over the frame's first or last column or row -- the row's tail run among them -- through reflected coordinates
// (bayer_reflect), so nothing outside the width x height sites is read.  phase: nmi_bayer_device.h.
__global__ __launch_bounds__(256) void nmi_unpack_bayer16_kernel(const uint8_t *__restrict__ src, size_t pitch, int phase,
                                                                 uint16_t *__restrict__ gray16, int width, int height, int vec)
{
    constexpr int WC = 10;
    const int run = blockIdx.x * kUnpackLanes + (int)threadIdx.x;
    const int y = blockIdx.y * 4 + (int)threadIdx.y;
    const int x0 = run * 8;
    if (x0 >= width || y >= height) return;
    const int n = min(8, width - x0);
    uint32_t win[3][WC];
    if (x0 >= 1 && x0 + 8 < width && y >= 1 && y + 1 < height) {
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const uint16_t *row = reinterpret_cast<const uint16_t *>(src + (size_t)(y - 1 + r) * pitch) + x0;
            uint32_t m[4];
            __builtin_memcpy(m, row, 16);
            win[r][0] = row[-1];
            win[r][WC - 1] = row[8];
#pragma unroll
            for (int i = 0; i < 4; ++i) win[r][1 + 2 * i] = m[i] & 0xFFFFu, win[r][2 + 2 * i] = m[i] >> 16;
        }
    } else {
        int xi[WC];  // (columns past the reflected one belong to pixels beyond the row's end, which are not stored: any site of the row)
#pragma unroll
        for (int i = 0; i < WC; ++i) xi[i] = min(max(bayer_reflect(x0 - 1 + i, width), 0), width - 1);
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const uint16_t *row = reinterpret_cast<const uint16_t *>(src + (size_t)bayer_reflect(y - 1 + r, height) * pitch);
#pragma unroll
            for (int i = 0; i < WC; ++i) win[r][i] = row[xi[i]];
        }
    }
    const int pa = phase & 1, b = (y ^ (phase >> 1)) & 1;
    uint32_t o[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int i = k + 1;  // the site's window column; x0 is even, so its column parity is k & 1
        const uint32_t hs = win[1][i - 1] + win[1][i + 1], vs = win[0][i] + win[2][i];
        const uint32_t ds = win[0][i - 1] + win[0][i + 1] + win[2][i - 1] + win[2][i + 1];
        o[k / 2] |= bayer_gray(win[1][i], hs, vs, ds, (k ^ pa) & 1, b) << (16 * (k & 1));
    }
    store_run(gray16 + (size_t)y * width + x0, o, n, vec);
}

hipError_t launch_unpack(const uint8_t *src, int format, int64_t pitch, uint16_t *gray16, int width, int height, hipStream_t stream)
{
    if (!frame_needs_unpack(format) || width <= 0 || height <= 0 || pitch <= 0) return hipErrorInvalidValue;
    if (frame_is_bayer16(format) && (width < 2 || height < 2)) return hipErrorInvalidValue;
    const int runs = (width + 7) / 8;
    const dim3 grid((runs + kUnpackLanes - 1) / kUnpackLanes, (height + 3) / 4), block(kUnpackLanes, 4);
    const uintptr_t base = (uintptr_t)gray16;
    const int vec = (base % 16) == 0 && (width % 8) == 0 ? 2 : (base % 8) == 0 && (width % 4) == 0 ? 1 : 0;
    const size_t pb = (size_t)pitch;
    switch (format) {
    case NMI_FRAME_GRAY16_BE: hipLaunchKernelGGL((nmi_unpack_kernel<kBigEndian>), grid, block, 0, stream, src, pb, gray16, width, height, vec); break;
    case NMI_FRAME_MONO10P: hipLaunchKernelGGL((nmi_unpack_kernel<kMono10p>), grid, block, 0, stream, src, pb, gray16, width, height, vec); break;
    case NMI_FRAME_MONO12P: hipLaunchKernelGGL((nmi_unpack_kernel<kMono12p>), grid, block, 0, stream, src, pb, gray16, width, height, vec); break;
    case NMI_FRAME_RAW10: hipLaunchKernelGGL((nmi_unpack_kernel<kRaw10>), grid, block, 0, stream, src, pb, gray16, width, height, vec); break;
    case NMI_FRAME_RAW12: hipLaunchKernelGGL((nmi_unpack_kernel<kRaw12>), grid, block, 0, stream, src, pb, gray16, width, height, vec); break;
    default:  // a 16-bit mosaic; bit 0 of its phase: the red sites' column parity, bit 1: their row parity
        hipLaunchKernelGGL(nmi_unpack_bayer16_kernel, grid, block, 0, stream, src, pb, format - NMI_FRAME_BAYER16_RGGB, gray16, width, height, vec);
        break;
    }
    return hipGetLastError();
}

}  // namespace nmi
