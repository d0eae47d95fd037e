// nmi_tone.hip -- deep grey frames (NMI_FRAME_GRAY16, include/nmi_hip.h) to the 8-bit grey frame the warps read, through one
// uint8 [65536] table per frame:
//   nmi_tone_hist_kernel    the exact histogram of v = min(raw, M) over the source's pixels (PERCENTILE and EQUALIZE only)
//   nmi_tone_sums_kernel    moves the histogram aside (clearing it) and sums it per segment of 1024 levels
//   nmi_tone_table_kernel   the running sums -> the table and the {lo, hi} pair, a segment per workgroup
//   nmi_gray16_kernel       table[min(raw, M)] per source pixel, then the rounded F x F box average (F = 1: the value itself)
// All arithmetic is integer (the one fp64 quotient is corrected to the exact floor), so tests/helpers/tone_np.py equals it bit
// for bit.
// With a valid range (nmi_set_valid_range) the histogram and the conversion are instantiations of their own of the same kernel
// templates: nmi_tone_hist_kernel<true> counts the pixels with lo <= raw <= hi only, nmi_gray16_kernel<F, true> also writes the
// validity mask.  What the range adds stands under `if constexpr`, and the plain instantiations are what they were before the range
// existed, instruction for instruction (profiles/deep_templates/isa_vs_parent.txt).
//
// The histogram counts in a per-workgroup uint32 LDS histogram of 16384 bins (64 KiB; a count cannot wrap, a frame has fewer
// than 2^32 pixels) and adds its nonzero bins to the global one.  LDS atomics on one address cost a wave some 64 LDS cycles,
// not a trip to L2 each, so a flat frame -- every pixel one value -- stays close to noise; the global histogram then sees one
// atomic per workgroup and value.  Depths above 14 bits take one pass per quarter of the range (top two bits of v) over the
// pixels a lane holds in registers, and a workgroup skips the quarters none of its pixels is in: a 14-bit scene in a 16-bit
// container is one pass.  Measurements: profiles/deep/README.md.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nmi_hip.h"
#include "nmi_tone.h"
#include "nmi_tone_device.h"
#include "nmi_reduce_device.h"

namespace nmi {

namespace {

constexpr int kHistThreads = 256;
constexpr int kHistBins = 16384;       // LDS bins of one pass: v's low 14 bits
constexpr int kHistRun = 8;            // pixels a lane takes at a time: 16 bytes of a row
constexpr int kHistRunsPerLane = 2;    // runs a lane keeps in registers over the passes
constexpr int kHistMaxWorkgroups = 1024;
constexpr int kSegThreads = 256;                          // lanes of a table workgroup, four levels each
constexpr int kSegments = kToneLevels / (4 * kSegThreads);  // 64 segments of 1024 levels = kToneRecords
static_assert(kSegments == kToneRecords && kSegments == 64, "a wave scans the segments' records");

// WINDOW's rule (include/nmi_hip.h); the order of the cases makes hi == lo all 0.
__device__ __forceinline__ uint32_t tone_window(uint32_t v, uint32_t lo, uint32_t hi)
{
    if (v <= lo) return 0u;
    if (v >= hi) return 255u;
    const uint32_t span = hi - lo;
    return ((v - lo) * 255u + (span >> 1)) / span;
}

}  // namespace

// A workgroup takes chunks of 256 x 2 runs of 8 pixels of one row (work item = row * runs_per_row + run), usually one chunk: a
// lane loads its two runs once and keeps them in registers over the passes.  vec: every row starts on a 16-byte boundary (base
// and pitch), so a whole run comes in one load; otherwise, and for the last run of a row whose width is not a multiple of 8,
// 2-byte loads of just the pixels inside the frame.  The flush clears the bins it adds to the global histogram.
// Ranged (Range: uint32_t lo, uint32_t hi; else nothing): a pixel is counted (and seen, for the quarters) iff it is inside the
// frame and lo <= raw <= hi, tested on the raw half-word before the saturation: bit k of ok[r].
template <bool Ranged, class... Range>
__global__ __launch_bounds__(kHistThreads) void nmi_tone_hist_kernel(const uint8_t *__restrict__ src, size_t pitch, int width, int height,
                                                                     uint32_t vmax, int passes, int vec, Range... lo_hi,
                                                                     uint32_t *__restrict__ hist)
{
    static_assert(sizeof...(Range) == (Ranged ? 2 : 0), "RangeArgs<Ranged>'s members");
    const RangeArgs<Ranged> range{lo_hi...};
    __shared__ uint4 bins4[kHistBins / 4];
    __shared__ uint32_t quarters;  // bit q: a pixel of this chunk has v >> 14 == q
    uint32_t *bins = reinterpret_cast<uint32_t *>(bins4);
    const int tid = (int)threadIdx.x;
    const uint32_t runs_per_row = (uint32_t)(width + kHistRun - 1) / kHistRun;
    const uint32_t items = runs_per_row * (uint32_t)height;  // (< 2^32: a GRAY16 frame has fewer than 2^32 pixels)
    const uint32_t chunk = gridDim.x * (uint32_t)(kHistThreads * kHistRunsPerLane);
    for (int i = tid; i < kHistBins / 4; i += kHistThreads) bins4[i] = make_uint4(0u, 0u, 0u, 0u);
    for (uint32_t first = 0; first < items; first += chunk) {  // (uniform over the workgroup; `first` cannot wrap: items + chunk < 2^32)
        uint32_t w[kHistRunsPerLane][kHistRun / 2];  // pixel k of run r is half k % 2 of word k / 2
        int n[kHistRunsPerLane];
        uint32_t seen = 0;
        [[maybe_unused]] uint32_t ok[kHistRunsPerLane] = {};  // (Ranged)
#pragma unroll
        for (int r = 0; r < kHistRunsPerLane; ++r) {
            const uint32_t item = first + (blockIdx.x * kHistRunsPerLane + r) * kHistThreads + tid;
#pragma unroll
            for (int k = 0; k < kHistRun / 2; ++k) w[r][k] = 0u;
            n[r] = 0;
            if (item < items) {
                const int y = (int)(item / runs_per_row), x0 = (int)(item % runs_per_row) * kHistRun;
                n[r] = min(kHistRun, width - x0);
                const uint8_t *p = src + (size_t)y * pitch + (size_t)x0 * 2;
                if (vec && n[r] == kHistRun) {
                    __builtin_memcpy(w[r], __builtin_assume_aligned(p, 16), 16);
                } else {
                    const uint16_t *p16 = reinterpret_cast<const uint16_t *>(p);
#pragma unroll
                    for (int k = 0; k < kHistRun; ++k)
                        if (k < n[r]) w[r][k / 2] |= (uint32_t)p16[k] << (16 * (k % 2));
                }
            }
        }
#pragma unroll
        for (int r = 0; r < kHistRunsPerLane; ++r) {
#pragma unroll
            for (int k = 0; k < kHistRun; ++k) {  // saturate in place
                const uint32_t raw = (w[r][k / 2] >> (16 * (k % 2))) & 0xFFFFu;
                const uint32_t v = min(raw, vmax);
                w[r][k / 2] = (w[r][k / 2] & ~(0xFFFFu << (16 * (k % 2)))) | (v << (16 * (k % 2)));
                if constexpr (Ranged) {
                    if (k < n[r] && raw >= range.lo && raw <= range.hi) ok[r] |= 1u << k, seen |= 1u << (v >> 14);
                } else {
                    if (k < n[r]) seen |= 1u << (v >> 14);
                }
            }
        }
        uint32_t present = 1u;
        if (passes > 1) {
            present = quarters_present(&quarters, seen, tid);
        } else {
            __syncthreads();  // (the bins are clear: the first zeroing, or the flush of the chunk before)
        }
        for (int pass = 0; pass < passes; ++pass) {
            if (!((present >> pass) & 1u)) continue;  // (uniform over the workgroup)
#pragma unroll
            for (int r = 0; r < kHistRunsPerLane; ++r) {
#pragma unroll
                for (int k = 0; k < kHistRun; ++k) {
                    const uint32_t v = (w[r][k / 2] >> (16 * (k % 2))) & 0xFFFFu;
                    if constexpr (Ranged) {
                        if (((ok[r] >> k) & 1u) && (v >> 14) == (uint32_t)pass) atomicAdd(&bins[v & (kHistBins - 1)], 1u);
                    } else {
                        if (k < n[r] && (v >> 14) == (uint32_t)pass) atomicAdd(&bins[v & (kHistBins - 1)], 1u);
                    }
                }
            }
            __syncthreads();
            uint32_t *out = hist + pass * kHistBins;  // (index < passes * 16384 <= 65536)
#pragma unroll 4
            for (int i = tid; i < kHistBins / 4; i += kHistThreads) flush_bins_quad(bins4, out, i);
            __syncthreads();
        }
        __syncthreads();  // (quarters is read by all before the next chunk resets it)
    }
}

// The histogram's way to the table, in two kernels of 64 workgroups x 256 lanes; workgroup p has the segment of 1024 levels
// [1024 p, 1024 p + 1024), lane t four of them.  (One workgroup doing all of it takes 25 .. 43 us: a single CU's loads of the
// 256 KiB the atomics left in memory, profiles/deep/README.md.)
//
// nmi_tone_sums_kernel moves the counts to `copy`, leaves the histogram all zero for the next frame, and writes its segment's
// record: the (plateau-clipped) sum, the last occupied level, and the first occupied level with its clipped count.
__global__ __launch_bounds__(kSegThreads) void nmi_tone_sums_kernel(uint32_t *__restrict__ hist, uint32_t *__restrict__ copy,
                                                                    uint32_t *__restrict__ records, uint32_t clip)
{
    __shared__ uint32_t s_sum, s_last;
    __shared__ unsigned long long s_first;  // level << 32 | clipped count
    const int tid = (int)threadIdx.x, at = blockIdx.x * kSegThreads + tid;
    if (tid == 0) s_sum = 0u, s_last = 0u, s_first = ~0ull;
    const uint4 q = reinterpret_cast<const uint4 *>(hist)[at];
    reinterpret_cast<uint4 *>(copy)[at] = q;
    reinterpret_cast<uint4 *>(hist)[at] = make_uint4(0u, 0u, 0u, 0u);
    const uint32_t c[4] = {q.x, q.y, q.z, q.w};
    uint32_t sum = 0, last = 0;
    unsigned long long first = ~0ull;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t cc = min(c[k], clip);
        sum += cc;
        if (c[k] != 0u) {
            const uint32_t level = 4u * at + k;
            if (first == ~0ull) first = (unsigned long long)level << 32 | cc;
            last = level;
        }
    }
    __syncthreads();
    if (sum) atomicAdd(&s_sum, sum);
    if (first != ~0ull) atomicMin(&s_first, first), atomicMax(&s_last, last);
    __syncthreads();
    if (tid == 0)
        reinterpret_cast<uint4 *>(records)[blockIdx.x] = make_uint4(s_sum, s_last, (uint32_t)s_first, (uint32_t)(s_first >> 32));
}

namespace {

// The (clipped) running sum below this lane's four levels within its workgroup's segment, from the lane's counts q; all 256
// lanes call it.  wave_total: shared [kSegThreads / 64], free again on return.
__device__ __forceinline__ uint32_t segment_below(const uint4 q, uint32_t clip, int tid, uint32_t *wave_total)
{
    const int lane = tid & 63, wave = tid >> 6;
    const uint32_t s = min(q.x, clip) + min(q.y, clip) + min(q.z, clip) + min(q.w, clip);
    uint32_t v = s;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t u = __shfl_up(v, d);
        if (lane >= d) v += u;
    }
    if (lane == 63) wave_total[wave] = v;
    __syncthreads();
    uint32_t before = v - s;
    for (int w = 0; w < wave; ++w) before += wave_total[w];
    __syncthreads();
    return before;
}

}  // namespace

// nmi_tone_table_kernel writes its segment of the table.  Fixed modes (copy == nullptr) compute their entries at once.  From
// the counts: every workgroup reads the 64 records, scans their sums into the running sum below each segment, and takes the
// frame's total, first and last occupied level from them; PERCENTILE finds the segments in which the running sum crosses its
// two ranks and scans those for the levels (every workgroup for itself: 4 KiB each); EQUALIZE scans its own segment for the
// running sum at each of its levels.  Levels above M hold no pixel, so their running sum -- and entry -- is M's, which is the
// rule for an index i > M (v = min(i, M)).  A histogram that counted nothing (N == 0: a valid range no pixel of the frame is in)
// gives the table all 0 and the pair {0, 0}.
__global__ __launch_bounds__(kSegThreads) void nmi_tone_table_kernel(ToneSetting t, const uint32_t *__restrict__ copy,
                                                                     const uint32_t *__restrict__ records, uint8_t *__restrict__ lut,
                                                                     int32_t *__restrict__ window)
{
    __shared__ uint32_t seg_below[kSegments], seg_sum[kSegments], wave_total[kSegThreads / 64];
    __shared__ unsigned long long first_level;  // vmin << 32 | h'[vmin]
    __shared__ uint32_t last_level, all, cross[2], cut[2];
    const int tid = (int)threadIdx.x, lane = tid & 63, p = (int)blockIdx.x;
    const uint32_t M = (1u << t.bits) - 1u;
    const bool equalize = t.mode == NMI_TONE_EQUALIZE;
    const uint32_t clip = equalize && t.plateau > 0 ? (uint32_t)t.plateau : 0xFFFFFFFFu;
    const uint4 *c4 = reinterpret_cast<const uint4 *>(copy);
    uint32_t lo = 0, hi = M, c0 = 0, total = 0, below = 0;
    uint4 own = make_uint4(0u, 0u, 0u, 0u);
    if (copy) {
        if (tid == 0) first_level = ~0ull, last_level = 0u, cross[0] = cross[1] = 0u, cut[0] = 0u, cut[1] = M;
        __syncthreads();
        if (tid < kSegments) {  // (wave 0, lane = segment)
            const uint4 r = reinterpret_cast<const uint4 *>(records)[tid];  // sum, last, first count, first level
            uint32_t v = r.x;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const uint32_t u = __shfl_up(v, d);
                if (lane >= d) v += u;
            }
            seg_below[tid] = v - r.x;
            seg_sum[tid] = r.x;
            if (tid == kSegments - 1) all = v;
            if (r.w != 0xFFFFFFFFu) atomicMin(&first_level, (unsigned long long)r.w << 32 | r.z), atomicMax(&last_level, r.y);
        }
        __syncthreads();
        total = all;
        if (t.mode == NMI_TONE_PERCENTILE) {
            // lo: the smallest v with c[v] > k_lo; hi: the smallest v with c[v] >= N - k_hi (N = total, the pixels counted)
            const uint32_t k_lo = (uint32_t)((uint64_t)total * (uint32_t)t.p_lo / 10000u);
            const uint32_t rank_hi = total - (uint32_t)((uint64_t)total * (uint32_t)t.p_hi / 10000u);
            if (tid < kSegments && seg_sum[tid] != 0u) {
                const uint32_t b = seg_below[tid], e = b + seg_sum[tid];
                if (b <= k_lo && e > k_lo) cross[0] = (uint32_t)tid;
                if (b < rank_hi && e >= rank_hi) cross[1] = (uint32_t)tid;
            }
            __syncthreads();
#pragma unroll
            for (int side = 0; side < 2; ++side) {
                const uint32_t seg = cross[side];  // (uniform over the workgroup)
                const uint4 q = c4[seg * kSegThreads + tid];
                const uint32_t c[4] = {q.x, q.y, q.z, q.w};
                uint32_t run = seg_below[seg] + segment_below(q, 0xFFFFFFFFu, tid, wave_total);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const uint32_t before = run;
                    run += c[k];
                    if (side == 0 ? (before <= k_lo && run > k_lo) : (before < rank_hi && run >= rank_hi))
                        cut[side] = (seg * kSegThreads + tid) * 4u + k;
                }
            }
            __syncthreads();
            lo = cut[0], hi = cut[1];
        } else {  // EQUALIZE
            if (total != 0u) lo = (uint32_t)(first_level >> 32), hi = last_level, c0 = (uint32_t)first_level;
            own = c4[p * kSegThreads + tid];
            below = seg_below[p] + segment_below(own, clip, tid, wave_total);
        }
    } else if (t.mode == NMI_TONE_WINDOW) {
        lo = (uint32_t)t.lo, hi = (uint32_t)t.hi;
    }
    const bool nothing = copy && total == 0u;
    if (nothing) lo = 0u, hi = 0u;
    const uint32_t den = total - c0;  // EQUALIZE: T - c0
    const double inv_den = den ? 1.0 / (double)den : 0.0;
    const uint32_t h[4] = {own.x, own.y, own.z, own.w};
    const uint32_t at = (uint32_t)p * kSegThreads + tid;  // this lane's levels: 4 at .. 4 at + 3
    uint32_t c = below, word = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t v = min(4u * at + k, M);
        uint32_t out;
        switch (t.mode) {
        case NMI_TONE_SHIFT: out = v >> (t.bits - 8); break;
        case NMI_TONE_WINDOW:
        case NMI_TONE_PERCENTILE: out = tone_window(v, lo, hi); break;
        case NMI_TONE_EQUALIZE:
            c += min(h[k], clip);  // c'[i]
            out = (den == 0u || v < lo) ? 0u : floor_div((uint64_t)(c - c0) * 255u + (den >> 1), den, inv_den);
            break;
        default: out = t.d_lut[v]; break;  // TABLE
        }
        if (nothing) out = 0u;
        word |= out << (8 * k);
    }
    if (((uintptr_t)lut % 4) == 0) {
        reinterpret_cast<uint32_t *>(lut)[at] = word;
    } else {  // (a caller's table that is not 4-byte aligned)
#pragma unroll
        for (int k = 0; k < 4; ++k) lut[4u * at + k] = (uint8_t)(word >> (8 * k));
    }
    if (p == 0 && tid == 0 && window) window[0] = (int32_t)lo, window[1] = (int32_t)hi;
}

// A lane makes 4 adjacent grey pixels of one output row from 4 F pixels of each of its F source rows.  vec_in: every source
// row starts on an 8-byte boundary (base and pitch), so a row's 8 F bytes come in F 8-byte loads; otherwise, and for the last
// quad of a row whose width is not a multiple of 4, 2-byte loads of just the pixels inside the frame.  vec_out: width % 4 == 0
// and gray 4-byte aligned, one dword store; otherwise byte stores.
// Masked (Valid: uint32_t lo, uint32_t hi, const uint8_t *frame_mask, uint8_t *mask; else nothing): the lane also writes the quad
// of the validity mask, from the raw values it holds: mask pixel k is 1 iff each of its F x F source pixels has lo <= raw <= hi
// and, with a frame mask, frame_mask's byte there is nonzero (write_valid_quad; the two may be one buffer).  vec_out then also
// asks for 4-byte aligned masks.
template <int F, bool Masked, class... Valid>
__global__ __launch_bounds__(256) void nmi_gray16_kernel(const uint8_t *__restrict__ src, size_t pitch, const uint8_t *__restrict__ lut,
                                                         uint32_t vmax, uint8_t *__restrict__ gray, int width, int height, int vec_in,
                                                         int vec_out, Valid... range_and_masks)
{
    static_assert(sizeof...(Valid) == (Masked ? 4 : 0), "MaskArgs<Masked>'s members");
    const MaskArgs<Masked> valid{range_and_masks...};
    const int x0 = (blockIdx.x * 64 + (int)threadIdx.x) * 4;
    const int y = blockIdx.y * 4 + (int)threadIdx.y;
    if (x0 >= width || y >= height) return;
    const int n = min(4, width - x0);
    const uint8_t *row = src + (size_t)y * F * pitch + (size_t)x0 * (F * 2);
    uint32_t s[4] = {};
    [[maybe_unused]] uint32_t bad = 0;  // (Masked) bit k: a source pixel of output pixel k is outside the range
    if (vec_in && n == 4) {
#pragma unroll
        for (int r = 0; r < F; ++r) {
            uint32_t w[2 * F];  // source pixel i of the row is half i % 2 of word i / 2
            __builtin_memcpy(w, __builtin_assume_aligned(row + (size_t)r * pitch, 8), 8 * F);
#pragma unroll
            for (int i = 0; i < 4 * F; ++i) {
                const uint32_t raw = (w[i / 2] >> (16 * (i % 2))) & 0xFFFFu;
                s[i / F] += lut[min(raw, vmax)];
                if constexpr (Masked) bad |= (uint32_t)(raw < valid.lo || raw > valid.hi) << (i / F);
            }
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (k < n) {
#pragma unroll
                for (int r = 0; r < F; ++r) {
                    const uint16_t *p16 = reinterpret_cast<const uint16_t *>(row + (size_t)r * pitch) + k * F;
#pragma unroll
                    for (int j = 0; j < F; ++j) {
                        const uint32_t raw = p16[j];
                        s[k] += lut[min(raw, vmax)];
                        if constexpr (Masked) bad |= (uint32_t)(raw < valid.lo || raw > valid.hi) << k;
                    }
                }
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

hipError_t launch_tone_hist(const uint8_t *src, int64_t pitch, int width, int height, int bits, const ValidRange &range, uint32_t *hist,
                            hipStream_t stream)
{
    const long long items = (long long)((width + kHistRun - 1) / kHistRun) * height, per = kHistThreads * kHistRunsPerLane;
    const long long want = (items + per - 1) / per;  // one chunk per workgroup up to 2M pixels
    const int workgroups = (int)(want < 1 ? 1 : want > kHistMaxWorkgroups ? kHistMaxWorkgroups : want);
    const int passes = bits <= 14 ? 1 : bits == 15 ? 2 : 4;
    const int vec = ((uintptr_t)src % 16) == 0 && (pitch % 16) == 0;
    const uint32_t vmax = (1u << bits) - 1u;
    if (range.on()) {
        hipLaunchKernelGGL((nmi_tone_hist_kernel<true, uint32_t, uint32_t>), dim3(workgroups), dim3(kHistThreads), 0, stream, src, (size_t)pitch,
                           width, height, vmax, passes, vec, (uint32_t)range.lo, (uint32_t)range.hi, hist);
    } else {
        hipLaunchKernelGGL(nmi_tone_hist_kernel<false>, dim3(workgroups), dim3(kHistThreads), 0, stream, src, (size_t)pitch, width, height, vmax,
                           passes, vec, hist);
    }
    return hipGetLastError();
}

hipError_t launch_tone_table(const ToneSetting &t, uint32_t *hist, uint8_t *lut, int32_t *window, hipStream_t stream)
{
    uint32_t *copy = nullptr, *records = nullptr;
    if (t.from_frame()) {
        copy = hist + kToneLevels, records = copy + kToneLevels;
        const uint32_t clip = t.mode == NMI_TONE_EQUALIZE && t.plateau > 0 ? (uint32_t)t.plateau : 0xFFFFFFFFu;
        hipLaunchKernelGGL(nmi_tone_sums_kernel, dim3(kSegments), dim3(kSegThreads), 0, stream, hist, copy, records, clip);
    }
    hipLaunchKernelGGL(nmi_tone_table_kernel, dim3(kSegments), dim3(kSegThreads), 0, stream, t, copy, records, lut, window);
    return hipGetLastError();
}

hipError_t launch_gray16(const uint8_t *src, int64_t pitch, int factor, const uint8_t *lut, int bits, const ValidRange &range,
                         const uint8_t *frame_mask, uint8_t *gray, uint8_t *mask, int width, int height, hipStream_t stream)
{
    const uint32_t vmax = (1u << bits) - 1u;
    const QuadLaunch q = quad_launch(src, pitch, frame_mask, gray, mask, width, height);
    const uint32_t lo = (uint32_t)range.lo, hi = (uint32_t)range.hi;
    return launch_for_factor(factor, [&](auto f) {
        constexpr int F = decltype(f)::value;
        if (mask) {
            hipLaunchKernelGGL((nmi_gray16_kernel<F, true>), q.grid, q.block, 0, stream, src, (size_t)pitch, lut, vmax, gray, width, height,
                               q.vec_in, q.vec_out, lo, hi, frame_mask, mask);
        } else {
            hipLaunchKernelGGL((nmi_gray16_kernel<F, false>), q.grid, q.block, 0, stream, src, (size_t)pitch, lut, vmax, gray, width, height,
                               q.vec_in, q.vec_out);
        }
    });
}

}  // namespace nmi
