// nmi_clahe.hip -- NMI_TONE_CLAHE (include/nmi_hip.h, "Deep frames"): contrast-limited equalisation per tile of a tiles_x x
// tiles_y grid over a deep grey frame, and the blend of the four nearest tiles' tables per pixel:
//   nmi_clahe_hist_kernel     the exact histogram of v = min(raw, M) of every tile
//   nmi_clahe_table_kernel    a tile's clipped running sum and redistributed excess -> its table; clears its histogram
//   nmi_clahe_gray16_kernel   the blend per source pixel, then the rounded F x F box average (F = 1: the value itself)
// All arithmetic is integer (the one fp64 quotient is corrected to the exact floor), so tests/helpers/clahe_np.py equals it bit
// for bit.
// With a valid range (nmi_set_valid_range) the histogram and the conversion are instantiations of their own of the same kernel
// templates, as in nmi_tone.hip: nmi_clahe_hist_kernel<true> counts the pixels with lo <= raw <= hi only, nmi_clahe_gray16_kernel<F,
// true> also writes the validity mask.  The plain instantiations are what they were before the range existed, instruction for
// instruction (profiles/deep_templates/isa_vs_parent.txt).
//
// Tile column i holds the source columns x with ((2 x + 1) tiles_x) / (2 Ws) == i, that is [x0[i], x0[i + 1]) with x0[i] =
// ceil((2 Ws i - tiles_x) / (2 tiles_x)); rows likewise.  The host works the edges out once (clahe_grid) and the histogram kernel
// takes them by value, so a workgroup counts the pixels of one tile only and its LDS histogram goes to that tile's global one.
//
// The histogram counts as nmi_tone_hist_kernel does: a per-workgroup uint32 LDS histogram of 16384 bins, its nonzero bins added
// to the global one.  LDS atomics on one address cost a wave some 64 LDS cycles, not a trip to L2 each, so a flat tile -- every
// pixel one value -- stays close to noise, and the tile's global histogram sees one atomic per workgroup and value.  Depths above
// 14 bits take one pass per quarter of the range over the pixels a lane holds in registers, and a workgroup skips the quarters
// none of its pixels is in; up to 14 bits a workgroup counts all its chunks before its one flush.  Measurements:
// profiles/clahe/README.md.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nmi_hip.h"
#include "nmi_tone.h"
#include "nmi_tone_device.h"
#include "nmi_reduce_device.h"

namespace nmi {

namespace {

constexpr int kHistThreads = 256;
constexpr int kHistBins = 16384;     // LDS bins of one pass: v's low 14 bits
constexpr int kHistPerLane = 16;     // pixels a lane keeps in registers over the passes, two to a word
constexpr int kHistChunk = kHistThreads * kHistPerLane;
constexpr int kHistMaxWorkgroups = 1024;
constexpr int kTableThreads = 1024;  // lanes of a table workgroup, four levels each a round
constexpr int kTableWaves = kTableThreads / 64;

// The edges of the tiles: tile column i is the source columns [x0[i], x0[i + 1]), tile row j the rows [y0[j], y0[j + 1]).
struct ClaheGrid {
    int32_t tx, ty;
    int32_t x0[kClaheMaxTiles + 1], y0[kClaheMaxTiles + 1];
};

void clahe_edges(int tiles, int size, int32_t *edge)
{
    edge[0] = 0;
    for (int i = 1; i < tiles; ++i) edge[i] = (int32_t)((2ll * size * i - tiles + 2ll * tiles - 1) / (2ll * tiles));
    for (int i = tiles; i <= kClaheMaxTiles; ++i) edge[i] = size;
}

ClaheGrid clahe_grid(int tx, int ty, int width, int height)
{
    ClaheGrid g{};
    g.tx = tx, g.ty = ty;
    clahe_edges(tx, width, g.x0);
    clahe_edges(ty, height, g.y0);
    return g;
}

}  // namespace

// Workgroup (c, t) counts chunks c, c + gridDim.x, ... of 256 x 16 pixels of tile t = blockIdx.y, pixel p of a tile being row
// p / tile width, column p % tile width of it.  2-byte loads: a tile's rows start wherever its edge falls.  The flush clears the
// bins it adds to the tile's global histogram.
// Ranged (Range: uint32_t lo, uint32_t hi; else nothing): a pixel is held (and seen, for the quarters) iff it is inside the tile
// and lo <= raw <= hi, tested on the raw half-word before the saturation.
template <bool Ranged, class... Range>
__global__ __launch_bounds__(kHistThreads) void nmi_clahe_hist_kernel(const uint8_t *__restrict__ src, size_t pitch, ClaheGrid g, uint32_t vmax,
                                                                      int bits, int passes, Range... lo_hi, uint32_t *__restrict__ hist)
{
    static_assert(sizeof...(Range) == (Ranged ? 2 : 0), "RangeArgs<Ranged>'s members");
    const RangeArgs<Ranged> range{lo_hi...};
    __shared__ uint4 bins4[kHistBins / 4];
    __shared__ uint32_t quarters;  // bit q: a pixel of this chunk has v >> 14 == q
    uint32_t *bins = reinterpret_cast<uint32_t *>(bins4);
    const int tid = (int)threadIdx.x;
    const int tile = (int)blockIdx.y, ti = tile % g.tx, tj = tile / g.tx;  // (tile < tx * ty: the launch's grid)
    const uint32_t x0 = (uint32_t)g.x0[ti], tw = (uint32_t)g.x0[ti + 1] - x0;
    const uint32_t y0 = (uint32_t)g.y0[tj], th = (uint32_t)g.y0[tj + 1] - y0;
    const uint64_t n = (uint64_t)tw * th;  // (< 2^32: a GRAY16 frame has fewer than 2^32 pixels)
    const int used4 = (bits < 14 ? (1 << bits) : kHistBins) / 4;  // the bins v can reach, in quads
    uint32_t *tile_hist = hist + ((size_t)tile << bits);
    for (int i = tid; i < used4; i += kHistThreads) bins4[i] = make_uint4(0u, 0u, 0u, 0u);
    __syncthreads();
    for (uint64_t first = (uint64_t)blockIdx.x * kHistChunk; first < n; first += (uint64_t)gridDim.x * kHistChunk) {  // (uniform)
        uint32_t w[kHistPerLane / 2];  // pixel k is half k % 2 of word k / 2, saturated
        uint32_t have = 0, seen = 0;   // bit k: pixel k is inside the tile (Ranged: and the range)
#pragma unroll
        for (int k = 0; k < kHistPerLane / 2; ++k) w[k] = 0u;
#pragma unroll
        for (int k = 0; k < kHistPerLane; ++k) {
            const uint64_t p = first + (uint64_t)(k * kHistThreads + tid);
            if (p < n) {
                const uint32_t row = (uint32_t)p / tw, col = (uint32_t)p - row * tw;  // row < th, col < tw: inside the frame
                const uint16_t raw = *reinterpret_cast<const uint16_t *>(src + (size_t)(y0 + row) * pitch + (size_t)(x0 + col) * 2);
                const uint32_t v = min((uint32_t)raw, vmax);
                if constexpr (Ranged) {
                    if ((uint32_t)raw < range.lo || (uint32_t)raw > range.hi) continue;  // not counted, not seen
                }
                w[k / 2] |= v << (16 * (k % 2));
                have |= 1u << k;
                seen |= 1u << (v >> 14);
            }
        }
        uint32_t present = 1u;
        if (passes > 1) present = quarters_present(&quarters, seen, tid);
        for (int pass = 0; pass < passes; ++pass) {
            if (!((present >> pass) & 1u)) continue;  // (uniform over the workgroup)
#pragma unroll
            for (int k = 0; k < kHistPerLane; ++k) {
                const uint32_t v = (w[k / 2] >> (16 * (k % 2))) & 0xFFFFu;
                if (((have >> k) & 1u) && (v >> 14) == (uint32_t)pass) atomicAdd(&bins[v & (kHistBins - 1)], 1u);
            }
            if (passes == 1) continue;  // one flush behind the last chunk
            __syncthreads();
            uint32_t *out = tile_hist + pass * kHistBins;  // (index < passes * 16384 <= 2^bits)
            for (int i = tid; i < kHistBins / 4; i += kHistThreads) flush_bins_quad(bins4, out, i);
            __syncthreads();
        }
        __syncthreads();  // (quarters is read by all before the next chunk resets it)
    }
    if (passes == 1) {
        __syncthreads();
        for (int i = tid; i < used4; i += kHistThreads) {  // (index < 4 used4 <= 2^bits)
            const uint4 c = bins4[i];
            if (c.x) atomicAdd(&tile_hist[4 * i], c.x);
            if (c.y) atomicAdd(&tile_hist[4 * i + 1], c.y);
            if (c.z) atomicAdd(&tile_hist[4 * i + 2], c.z);
            if (c.w) atomicAdd(&tile_hist[4 * i + 3], c.w);
        }
    }
}

namespace {

// The sum of x over the workgroup's kTableThreads lanes; all call it.  part: shared [kTableWaves], free again on return.
__device__ __forceinline__ uint32_t table_sum(uint32_t x, int tid, uint32_t *part)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) x += __shfl_xor(x, d);
    if ((tid & 63) == 0) part[tid >> 6] = x;
    __syncthreads();
    uint32_t all = 0;
#pragma unroll
    for (int w = 0; w < kTableWaves; ++w) all += part[w];
    __syncthreads();
    return all;
}

}  // namespace

// One workgroup per tile, rounds of 4096 levels, lane t the four levels 4096 round + 4 t ...  A first walk over the tile's
// histogram gives its pixel count n and the excess E over the plateau; the second clears it and scans the clipped counts, the
// running sum carried from round to round, and writes the table: c''[v] = c'[v] + q (v + 1) + (r ? min(r, v / step + 1) : 0)
// with q = E / L, r = E % L, step = max(L / r, 1), then (c''[v] 255 + (n >> 1)) / n.  Entries above M take M's.  n is the
// histogram's sum; n == 0 (a ranged histogram of a tile with no valid pixel): SHIFT's table, v >> (bits - 8).
__global__ __launch_bounds__(kTableThreads) void nmi_clahe_table_kernel(uint32_t *__restrict__ hist, int bits, uint32_t plateau,
                                                                        uint8_t *__restrict__ luts, uint32_t *__restrict__ counts)
{
    __shared__ uint32_t part[kTableWaves];
    __shared__ uint32_t top;  // the entry of level M
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, tile = (int)blockIdx.x;
    const uint32_t L = 1u << bits, M = L - 1u;
    const uint32_t clip = plateau > 0u ? plateau : 0xFFFFFFFFu;
    uint4 *h4 = reinterpret_cast<uint4 *>(hist + ((size_t)tile << bits));
    uint32_t *lut4 = reinterpret_cast<uint32_t *>(luts + (size_t)tile * kToneLevels);
    const int rounds = (int)((L + 4u * kTableThreads - 1u) / (4u * kTableThreads));
    uint32_t sum = 0, over = 0;
    for (int k = 0; k < rounds; ++k) {
        const uint32_t at = (uint32_t)k * kTableThreads + tid;  // this lane's levels: 4 at .. 4 at + 3
        if (4u * at < L) {
            const uint4 q = h4[at];
            sum += q.x + q.y + q.z + q.w;
            over += (q.x - min(q.x, clip)) + (q.y - min(q.y, clip)) + (q.z - min(q.z, clip)) + (q.w - min(q.w, clip));
        }
    }
    const uint32_t n = table_sum(sum, tid, part);  // (> 0 unless the histogram was a ranged one: no tile is empty)
    const uint32_t E = table_sum(over, tid, part);
    const uint32_t q = E >> bits, r = E & M, step = r ? max(L / r, 1u) : 1u;
    if (n == 0u) {  // (uniform) nothing counted: SHIFT's table; the histogram is all zero already
        for (uint32_t at = tid; at < (uint32_t)kToneLevels / 4u; at += kTableThreads) {
            uint32_t word = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i) word |= (min(4u * at + i, M) >> (bits - 8)) << (8 * i);
            lut4[at] = word;
        }
        if (tid == 0) counts[tile] = 0u;
        return;
    }
    const double inv_n = 1.0 / (double)n;
    uint32_t carry = 0;  // c' below this round
    for (int k = 0; k < rounds; ++k) {
        const uint32_t at = (uint32_t)k * kTableThreads + tid;
        const bool valid = 4u * at < L;
        uint4 own = make_uint4(0u, 0u, 0u, 0u);
        if (valid) {
            own = h4[at];
            h4[at] = make_uint4(0u, 0u, 0u, 0u);  // zero for the next frame
        }
        const uint32_t h[4] = {min(own.x, clip), min(own.y, clip), min(own.z, clip), min(own.w, clip)};
        const uint32_t s = h[0] + h[1] + h[2] + h[3];
        uint32_t v = s;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t u = __shfl_up(v, d);
            if (lane >= d) v += u;
        }
        if (lane == 63) part[wave] = v;
        __syncthreads();
        uint32_t c = carry + v - s, total = 0;
#pragma unroll
        for (int w = 0; w < kTableWaves; ++w) {
            const uint32_t pw = part[w];
            if (w < wave) c += pw;
            total += pw;
        }
        carry += total;
        if (valid) {
            uint32_t word = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const uint32_t level = 4u * at + i;
                c += h[i];  // c'[level]
                const uint64_t cc = (uint64_t)c + (uint64_t)q * (level + 1u) + (r ? min(r, level / step + 1u) : 0u);  // (<= n)
                const uint32_t out = floor_div(cc * 255u + (n >> 1), n, inv_n);
                word |= out << (8 * i);
                if (level == M) top = out;
            }
            lut4[at] = word;
        }
        __syncthreads();  // (part is free again; top is written before the fill below)
    }
    const uint32_t fill = top * 0x01010101u;
    for (uint32_t at = L / 4u + tid; at < (uint32_t)kToneLevels / 4u; at += kTableThreads) lut4[at] = fill;
    if (tid == 0) counts[tile] = n;
}

namespace {

// Where source coordinate x lies between the tile centres of an axis of `size` pixels in `tiles` tiles: lower tile | upper tile
// << 8 | weight of the upper << 16, both tiles clamped to the grid.  With u = (2 x + 1) tiles + size, the rule's ax + dx, one
// quotient 256 u / dx holds both: its high part is i0 + 1, its low byte wx.  wide: 4352 size does not fit 32 bits.
__device__ __forceinline__ uint32_t clahe_axis(uint32_t x, uint32_t tiles, uint32_t size, int wide)
{
    uint32_t g;
    if (wide) {
        g = (uint32_t)((((uint64_t)(2u * x + 1u) * tiles + size) * 256u) / (2ull * size));
    } else {
        g = (((2u * x + 1u) * tiles + size) * 256u) / (2u * size);
    }
    const int i0 = (int)(g >> 8) - 1;  // -1 .. tiles - 1
    const uint32_t lo = (uint32_t)max(i0, 0), hi = min((uint32_t)(i0 + 1), tiles - 1u);
    return lo | hi << 8 | (g & 255u) << 16;
}

}  // namespace

// nmi_gray16_kernel's shape: a lane makes 4 adjacent grey pixels of one output row from 4 F pixels of each of its F source rows,
// loaded first (vec_in: 8-byte loads, every source row starting on an 8-byte boundary; otherwise, and for the last quad of a row
// whose width is not a multiple of 4, 2-byte loads of just the pixels inside the frame), then taken column by column: a column's
// tile pair and weight once, four gathers and the blend for each of its F pixels.  luts: [tiles_y][tiles_x][65536].
// Masked (Valid: uint32_t lo, uint32_t hi, const uint8_t *frame_mask, uint8_t *mask; else nothing): the lane also writes the quad
// of the validity mask, as nmi_gray16_kernel<F, true> does (write_valid_quad); vec_out then also asks for 4-byte aligned masks.
template <int F, bool Masked, class... Valid>
__global__ __launch_bounds__(256) void nmi_clahe_gray16_kernel(const uint8_t *__restrict__ src, size_t pitch, const uint8_t *__restrict__ luts,
                                                               uint32_t vmax, uint32_t tiles_x, uint32_t tiles_y, uint8_t *__restrict__ gray,
                                                               int width, int height, int vec_in, int vec_out, int wide,
                                                               Valid... range_and_masks)
{
    static_assert(sizeof...(Valid) == (Masked ? 4 : 0), "MaskArgs<Masked>'s members");
    const MaskArgs<Masked> valid{range_and_masks...};
    const int x0 = (blockIdx.x * 64 + (int)threadIdx.x) * 4;
    const int y = blockIdx.y * 4 + (int)threadIdx.y;
    if (x0 >= width || y >= height) return;
    const int n = min(4, width - x0);
    const uint8_t *row = src + (size_t)y * F * pitch + (size_t)x0 * (F * 2);
    uint32_t w[F][2 * F] = {};  // source pixel i of row r is half i % 2 of word i / 2
    if (vec_in && n == 4) {
#pragma unroll
        for (int r = 0; r < F; ++r) __builtin_memcpy(w[r], __builtin_assume_aligned(row + (size_t)r * pitch, 8), 8 * F);
    } else {
#pragma unroll
        for (int r = 0; r < F; ++r) {
            const uint16_t *p16 = reinterpret_cast<const uint16_t *>(row + (size_t)r * pitch);
#pragma unroll
            for (int i = 0; i < 4 * F; ++i)
                if (i < n * F) w[r][i / 2] |= (uint32_t)p16[i] << (16 * (i % 2));
        }
    }
    uint32_t rows[F];
#pragma unroll
    for (int r = 0; r < F; ++r) rows[r] = clahe_axis((uint32_t)(y * F + r), tiles_y, (uint32_t)height * F, wide);
    uint32_t s[4] = {};
    [[maybe_unused]] uint32_t bad = 0;  // (Masked) bit k: a source pixel of output pixel k is outside the range
#pragma unroll
    for (int i = 0; i < 4 * F; ++i) {
        if (i < n * F) {
            const uint32_t cx = clahe_axis((uint32_t)(x0 * F + i), tiles_x, (uint32_t)width * F, wide);
            const uint32_t i0 = cx & 255u, i1 = (cx >> 8) & 255u, wx = cx >> 16;
#pragma unroll
            for (int r = 0; r < F; ++r) {
                const uint32_t raw = (w[r][i / 2] >> (16 * (i % 2))) & 0xFFFFu;
                const uint32_t v = min(raw, vmax);
                if constexpr (Masked) bad |= (uint32_t)(raw < valid.lo || raw > valid.hi) << (i / F);
                const uint32_t j0 = rows[r] & 255u, j1 = (rows[r] >> 8) & 255u, wy = rows[r] >> 16;
                const uint8_t *t0 = luts + ((size_t)(j0 * tiles_x) << 16) + v, *t1 = luts + ((size_t)(j1 * tiles_x) << 16) + v;
                const uint32_t A = t0[(size_t)i0 << 16], B = t0[(size_t)i1 << 16], C = t1[(size_t)i0 << 16], D = t1[(size_t)i1 << 16];
                const uint32_t up = A * (256u - wx) + B * wx, down = C * (256u - wx) + D * wx;
                s[i / F] += (up * (256u - wy) + down * wy + 32768u) >> 16;
            }
        }
    }
    uint32_t packed = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) packed |= reduce_round<F>(s[k]) << (8 * k);
    const size_t o = (size_t)y * width + x0;
    if (vec_out) {  // (width % 4 == 0: the quad lies wholly inside the row)
        *reinterpret_cast<uint32_t *>(gray + o) = packed;
    } else {
        for (int k = 0; k < n; ++k) gray[o + k] = (uint8_t)(packed >> (8 * k));
    }
    if constexpr (Masked) write_valid_quad(bad, valid.frame_mask, valid.mask, o, n, vec_out);
}

hipError_t launch_clahe_hist(const ToneSetting &t, const uint8_t *src, int64_t pitch, int width, int height, const ValidRange &range,
                             uint32_t *hist, hipStream_t stream)
{
    const ClaheGrid g = clahe_grid(t.tiles_x, t.tiles_y, width, height);
    const int tiles = t.tiles_x * t.tiles_y;
    // the largest tile's chunks, one workgroup each until the grid would pass kHistMaxWorkgroups
    const long long widest = (long long)(width + t.tiles_x - 1) / t.tiles_x + 1, tallest = (long long)(height + t.tiles_y - 1) / t.tiles_y + 1;
    const long long chunks = (widest * tallest + kHistChunk - 1) / kHistChunk, most = kHistMaxWorkgroups / tiles;
    const int per_tile = (int)(chunks < most ? chunks : most);
    const int passes = t.bits <= 14 ? 1 : t.bits == 15 ? 2 : 4;
    const uint32_t vmax = (1u << t.bits) - 1u;
    if (range.on()) {
        hipLaunchKernelGGL((nmi_clahe_hist_kernel<true, uint32_t, uint32_t>), dim3(per_tile, tiles), dim3(kHistThreads), 0, stream, src,
                           (size_t)pitch, g, vmax, t.bits, passes, (uint32_t)range.lo, (uint32_t)range.hi, hist);
    } else {
        hipLaunchKernelGGL(nmi_clahe_hist_kernel<false>, dim3(per_tile, tiles), dim3(kHistThreads), 0, stream, src, (size_t)pitch, g, vmax, t.bits,
                           passes, hist);
    }
    return hipGetLastError();
}

hipError_t launch_clahe_tables(const ToneSetting &t, uint32_t *hist, uint8_t *luts, uint32_t *counts, hipStream_t stream)
{
    hipLaunchKernelGGL(nmi_clahe_table_kernel, dim3(t.tiles_x * t.tiles_y), dim3(kTableThreads), 0, stream, hist, t.bits, (uint32_t)t.plateau,
                       luts, counts);
    return hipGetLastError();
}

hipError_t launch_clahe_gray16(const ToneSetting &t, const uint8_t *src, int64_t pitch, int factor, const uint8_t *luts, const ValidRange &range,
                               const uint8_t *frame_mask, uint8_t *gray, uint8_t *mask, int width, int height, hipStream_t stream)
{
    const uint32_t vmax = (1u << t.bits) - 1u, tx = (uint32_t)t.tiles_x, ty = (uint32_t)t.tiles_y;
    const QuadLaunch q = quad_launch(src, pitch, frame_mask, gray, mask, width, height);
    const uint32_t lo = (uint32_t)range.lo, hi = (uint32_t)range.hi;
    return launch_for_factor(factor, [&](auto f) {
        constexpr int F = decltype(f)::value;
        const int wide = (long long)width * F >= (1 << 19) || (long long)height * F >= (1 << 19);  // 4352 * 2^19 < 2^32
        if (mask) {
            hipLaunchKernelGGL((nmi_clahe_gray16_kernel<F, true>), q.grid, q.block, 0, stream, src, (size_t)pitch, luts, vmax, tx, ty, gray, width,
                               height, q.vec_in, q.vec_out, wide, lo, hi, frame_mask, mask);
        } else {
            hipLaunchKernelGGL((nmi_clahe_gray16_kernel<F, false>), q.grid, q.block, 0, stream, src, (size_t)pitch, luts, vmax, tx, ty, gray, width,
                               height, q.vec_in, q.vec_out, wide);
        }
    });
}

}  // namespace nmi
