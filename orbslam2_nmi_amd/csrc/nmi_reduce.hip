// nmi_reduce.hip -- full-size camera frames to the dense grey frame of the search size (nmi_reduce_frame, include/nmi_hip.h):
// every source pixel turned grey by nmi_gray_frame's rule (nmi_color_device.h), then the rounded box average of each F x F
// block, F = 2, 3 or 4 (F = 1 is nmi_color.hip; a Bayer mosaic, whose pixels need their neighbours, is nmi_bayer.hip at every
// F).  The kernel moves a frame's bytes once -- 1920x1080 RGB is 6.2 MB in and 0.5 MB
// out -- with no LDS and no reuse between lanes.  The mask instantiation makes the reduced frame mask: 1 where a whole block of
// the source mask is nonzero.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nmi_hip.h"
#include "nmi_color.h"
#include "nmi_color_device.h"
#include "nmi_reduce.h"
#include "nmi_reduce_device.h"

namespace nmi {

namespace {

constexpr int kReduceLanes = 64;  // lanes per block row; 4 block rows (the conversion kernel's shape)

// Output pixels a lane makes: the shortest run of 4, 8 or 16 whose source bytes per row, run * F * C, are whole 16-byte loads.
template <int C, int F>
constexpr int reduce_run()
{
    return (4 * F * C) % 16 == 0 ? 4 : (8 * F * C) % 16 == 0 ? 8 : 16;
}

// What one source pixel adds to its block's sum: its grey value, or (MASK) 1 for a nonzero mask byte.
template <int C, int RI, bool MASK>
__device__ __forceinline__ uint32_t reduce_term(const uint8_t *p)
{
    if constexpr (MASK)
        return p[0] != 0 ? 1u : 0u;
    else
        return color_pixel<C, RI>(p);
}

template <int F, bool MASK>
__device__ __forceinline__ uint32_t reduce_value(uint32_t s)
{
    if constexpr (MASK)
        return s == (uint32_t)(F * F) ? 1u : 0u;
    else
        return reduce_round<F>(s);
}

}  // namespace

// A lane makes N = reduce_run<C, F>() adjacent pixels of one output row from N * F * C bytes of each of its F source rows.
// vec_in: every source row starts on a 16-byte boundary (base and pitch), so each row's bytes come in 16-byte loads; otherwise,
// and for the last run of a row whose width is not a multiple of N, byte loads of just the pixels inside the frame.  vec_out:
// width % N == 0 and out N-byte aligned, one store of N bytes (a dword, two or four); otherwise byte stores.
template <int C, int RI, int F, bool MASK>
__global__ __launch_bounds__(256) void nmi_reduce_kernel(const uint8_t *__restrict__ src, size_t pitch, uint8_t *__restrict__ out, int width,
                                                         int height, int vec_in, int vec_out)
{
    constexpr int N = reduce_run<C, F>(), B = N * F * C;
    const int x0 = (blockIdx.x * kReduceLanes + (int)threadIdx.x) * N;
    const int y = blockIdx.y * 4 + (int)threadIdx.y;
    if (x0 >= width || y >= height) return;
    const int n = min(N, width - x0);
    const uint8_t *row = src + (size_t)y * F * pitch + (size_t)x0 * (F * C);
    uint32_t packed[N / 4] = {};
    if (vec_in && n == N) {
        uint8_t b[F][B];  // pixel j of output k in row r starts at byte (k * F + j) * C of b[r]
#pragma unroll
        for (int r = 0; r < F; ++r) {
            uint32_t w[B / 4];
            __builtin_memcpy(w, __builtin_assume_aligned(row + (size_t)r * pitch, 16), B);
#pragma unroll
            for (int i = 0; i < B; ++i) b[r][i] = (uint8_t)(w[i / 4] >> (8 * (i % 4)));
        }
#pragma unroll
        for (int k = 0; k < N; ++k) {
            uint32_t s = 0;
#pragma unroll
            for (int r = 0; r < F; ++r)
#pragma unroll
                for (int j = 0; j < F; ++j) s += reduce_term<C, RI, MASK>(&b[r][(k * F + j) * C]);
            packed[k / 4] |= reduce_value<F, MASK>(s) << (8 * (k % 4));
        }
    } else {
#pragma unroll
        for (int k = 0; k < N; ++k) {
            if (k < n) {
                uint32_t s = 0;
#pragma unroll
                for (int r = 0; r < F; ++r)
#pragma unroll
                    for (int j = 0; j < F; ++j) s += reduce_term<C, RI, MASK>(row + (size_t)r * pitch + (k * F + j) * C);
                packed[k / 4] |= reduce_value<F, MASK>(s) << (8 * (k % 4));
            }
        }
    }
    uint8_t *o = out + (size_t)y * width + x0;
    if (vec_out) {  // (width % N == 0: the run lies wholly inside the row)
        __builtin_memcpy(__builtin_assume_aligned(o, N), packed, N);
    } else {
#pragma unroll
        for (int k = 0; k < N; ++k)
            if (k < n) o[k] = (uint8_t)(packed[k / 4] >> (8 * (k % 4)));
    }
}

namespace {

template <int C, int RI, int F, bool MASK>
void reduce_launch(const uint8_t *src, size_t pitch, uint8_t *out, int width, int height, hipStream_t stream)
{
    constexpr int N = reduce_run<C, F>();
    const int runs = (width + N - 1) / N;
    const dim3 grid((runs + kReduceLanes - 1) / kReduceLanes, (height + 3) / 4), block(kReduceLanes, 4);
    const int vec_in = ((uintptr_t)src % 16) == 0 && (pitch % 16) == 0;
    const int vec_out = (width % N) == 0 && ((uintptr_t)out % N) == 0;
    hipLaunchKernelGGL((nmi_reduce_kernel<C, RI, F, MASK>), grid, block, 0, stream, src, pitch, out, width, height, vec_in, vec_out);
}

template <int C, int RI, bool MASK>
bool reduce_by_factor(int factor, const uint8_t *src, size_t pitch, uint8_t *out, int width, int height, hipStream_t stream)
{
    switch (factor) {
    case 1:  // the mask alone: a frame at factor 1 is launch_gray's
        if constexpr (MASK) reduce_launch<C, RI, 1, MASK>(src, pitch, out, width, height, stream);
        return MASK;
    case 2: reduce_launch<C, RI, 2, MASK>(src, pitch, out, width, height, stream); return true;
    case 3: reduce_launch<C, RI, 3, MASK>(src, pitch, out, width, height, stream); return true;
    case 4: reduce_launch<C, RI, 4, MASK>(src, pitch, out, width, height, stream); return true;
    default: return false;
    }
}

}  // namespace

hipError_t launch_reduce(const uint8_t *src, int format, int64_t pitch, int factor, uint8_t *gray, int width, int height, hipStream_t stream)
{
    if (frame_is_bayer(format)) return launch_bayer(src, format, pitch, factor, gray, width, height, stream);
    const size_t pb = (size_t)pitch;
    bool known = false;
    switch (format) {
    case NMI_FRAME_YUYV: known = reduce_by_factor<2, 0, false>(factor, src, pb, gray, width, height, stream); break;
    case NMI_FRAME_UYVY: known = reduce_by_factor<2, 1, false>(factor, src, pb, gray, width, height, stream); break;
    case NMI_FRAME_GRAY: known = reduce_by_factor<1, 0, false>(factor, src, pb, gray, width, height, stream); break;
    case NMI_FRAME_BGR: known = reduce_by_factor<3, 2, false>(factor, src, pb, gray, width, height, stream); break;
    case NMI_FRAME_RGB: known = reduce_by_factor<3, 0, false>(factor, src, pb, gray, width, height, stream); break;
    case NMI_FRAME_BGRA: known = reduce_by_factor<4, 2, false>(factor, src, pb, gray, width, height, stream); break;
    case NMI_FRAME_RGBA: known = reduce_by_factor<4, 0, false>(factor, src, pb, gray, width, height, stream); break;
    default: break;
    }
    return known ? hipGetLastError() : hipErrorInvalidValue;
}

hipError_t launch_reduce_mask(const uint8_t *src_mask, int factor, uint8_t *mask, int width, int height, hipStream_t stream)
{
    const bool known = reduce_by_factor<1, 0, true>(factor, src_mask, (size_t)factor * (size_t)width, mask, width, height, stream);
    return known ? hipGetLastError() : hipErrorInvalidValue;
}

}  // namespace nmi
