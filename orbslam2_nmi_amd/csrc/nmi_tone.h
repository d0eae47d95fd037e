// nmi_tone.h -- internal interface of the deep grey frames (NMI_FRAME_GRAY16, include/nmi_hip.h): the tone map as a checked
// value, the device buffers that go with it, and the kernels of nmi_tone.hip.  Every mode goes through one uint8 [65536] table:
// the fixed modes' (SHIFT, WINDOW) is built when the setting changes, the data-dependent ones' (PERCENTILE, EQUALIZE) by two
// kernels in front of every conversion, and TABLE's is the caller's.  Used by nmi_capi_tone.cpp (the entries), nmi_capi_color.cpp,
// nmi_capi_reduce.cpp and nmi_capi_intake.cpp (levels and streams, with a range of their own).
// CLAHE is the one mode with a table per tile, four of them blended per pixel: its kernels are nmi_clahe.hip's, its buffers
// ToneWork's tile_hist and tile_luts, and deep_gray() below is where a conversion takes one way or the other.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "nmi_hip.h"
#include "nmi_mem.h"

namespace nmi {

constexpr int kToneLevels = 65536;  // entries of a table, words of a histogram
constexpr int kToneRecords = 64;    // segments of 1024 levels the table kernels work by, a 4-word record each
// Words of a histogram buffer: the histogram itself (zero between frames), its copy for the table kernel, the records.
constexpr size_t kToneHistWords = 2 * (size_t)kToneLevels + 4 * kToneRecords;

// An nmi_tone_map that passed tone_check (nmi_capi_tone.cpp), as the table kernel takes it.
struct ToneSetting {
    int32_t mode = NMI_TONE_SHIFT, bits = 16;
    int32_t lo = 0, hi = 65535;      // WINDOW
    int32_t p_lo = 0, p_hi = 0;      // PERCENTILE
    int32_t plateau = 0;             // EQUALIZE, CLAHE
    int32_t tiles_x = 0, tiles_y = 0;  // CLAHE: 1 .. kClaheMaxTiles each (0 under every other mode)
    const uint8_t *d_lut = nullptr;  // TABLE: the caller's
    bool tiled() const { return mode == NMI_TONE_CLAHE; }
    bool from_frame() const { return mode == NMI_TONE_PERCENTILE || mode == NMI_TONE_EQUALIZE || mode == NMI_TONE_CLAHE; }
    bool operator==(const ToneSetting &o) const
    {
        return mode == o.mode && bits == o.bits && lo == o.lo && hi == o.hi && p_lo == o.p_lo && p_hi == o.p_hi && plateau == o.plateau &&
               tiles_x == o.tiles_x && tiles_y == o.tiles_y && d_lut == o.d_lut;
    }
};

// The valid range of a GRAY16 source (nmi_set_valid_range; a level's and a stream's own: nmi_level_set_valid_range,
// nmi_stream_set_valid_range): a pixel counts in the statistics, and is 1 in the validity mask, iff lo <= raw <= hi, raw being
// the container's value before it saturates to 2^bits - 1.  (0, 65535): off, and the histogram launches below then launch the
// plain instantiation of their kernel.
struct ValidRange {
    int32_t lo = 0, hi = 65535;
    bool on() const { return lo != 0 || hi != 65535; }
    bool operator==(const ValidRange &o) const { return lo == o.lo && hi == o.hi; }
};

// hist[v] += the number of pixels with min(raw, 2^bits - 1) == v and raw inside `range` among the height rows of pitch bytes at
// src, each width little-endian 16-bit pixels (src and pitch even).  Exact for any content; hist is uint32 [kToneLevels].  The
// ranged count is an instantiation of its own of the kernel, so range off launches what it did before the range existed.
hipError_t launch_tone_hist(const uint8_t *src, int64_t pitch, int width, int height, int bits, const ValidRange &range, uint32_t *hist,
                            hipStream_t stream);

// lut[i] = the setting's 8-bit value of min(i, 2^bits - 1) for all kToneLevels indices, and window[0 .. 1] = the {lo, hi} pair
// nmi_tone_lut reports (window may be null).  hist: for a from_frame() mode the frame's histogram at the head of a buffer of
// kToneHistWords words, left all zero for the next frame (two kernels); never read otherwise (one kernel).  N is the histogram's
// sum; N == 0 (a ranged histogram of a frame with no valid pixel): the table all 0, the window {0, 0}.
hipError_t launch_tone_table(const ToneSetting &t, uint32_t *hist, uint8_t *lut, int32_t *window, hipStream_t stream);

// nmi_gray_frame (factor 1) and nmi_reduce_frame (factor 2 .. 4) of a GRAY16 source of factor * height rows of pitch bytes,
// each factor * width pixels: lut[min(raw, 2^bits - 1)] per source pixel, then the rounded box average (nmi_reduce_device.h).
// lut is the table of launch_tone_table, or a TABLE setting's own.
// mask (may be null): the masked instantiation of the kernel, which also writes the validity mask: mask[y][x] = 1 iff all factor x
// factor source pixels under (x, y) are inside `range` and frame_mask[y][x] != 0 (frame_mask: dense [height][width], may be null,
// may be `mask` itself).  Without a mask neither `range` nor frame_mask is read.
hipError_t launch_gray16(const uint8_t *src, int64_t pitch, int factor, const uint8_t *lut, int bits, const ValidRange &range,
                         const uint8_t *frame_mask, uint8_t *gray, uint8_t *mask, int width, int height, hipStream_t stream);

// The launch geometry of the two conversions (launch_gray16, launch_clahe_gray16): a lane makes a quad of 4 adjacent grey pixels,
// a workgroup 64 quads of each of 4 rows.  vec_in: every source row starts on an 8-byte boundary (base and pitch); vec_out: width
// % 4 == 0 and the grey frame -- with a mask, the mask pair too -- 4-byte aligned.
struct QuadLaunch {
    dim3 grid, block;
    int vec_in, vec_out;
};
inline QuadLaunch quad_launch(const uint8_t *src, int64_t pitch, const uint8_t *frame_mask, uint8_t *gray, uint8_t *mask, int width, int height)
{
    const int quads = (width + 3) / 4;
    const dim3 grid((quads + 63) / 64, (height + 3) / 4), block(64, 4);
    const int vec_in = ((uintptr_t)src % 8) == 0 && (pitch % 8) == 0;
    const uintptr_t masks = mask ? (uintptr_t)mask | (uintptr_t)frame_mask : 0;
    const int vec_out = (width % 4) == 0 && (((uintptr_t)gray | masks) % 4) == 0;
    return {grid, block, vec_in, vec_out};
}

// launch(std::integral_constant<int, factor>{}) for a factor of 1 .. 4, then hipGetLastError(); hipErrorInvalidValue for any other.
template <class Launch>
hipError_t launch_for_factor(int factor, Launch &&launch)
{
    switch (factor) {
    case 1: launch(std::integral_constant<int, 1>{}); break;
    case 2: launch(std::integral_constant<int, 2>{}); break;
    case 3: launch(std::integral_constant<int, 3>{}); break;
    case 4: launch(std::integral_constant<int, 4>{}); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// --- CLAHE (nmi_clahe.hip; the rule: include/nmi_hip.h "Deep frames") ---------------------------------------------------------
constexpr int kClaheMaxTiles = 8;                                  // per axis
constexpr int kClaheMaxTileCount = kClaheMaxTiles * kClaheMaxTiles;
// Bytes of the tile histograms (uint32 [ty][tx][2^bits], zero between frames) and of the tile tables (uint8 [ty][tx][65536],
// then the tiles' pixel counts, uint32 [kClaheMaxTileCount]).
inline size_t clahe_hist_bytes(const ToneSetting &t) { return ((size_t)t.tiles_x * t.tiles_y << t.bits) * sizeof(uint32_t); }
inline size_t clahe_luts_bytes(const ToneSetting &t) { return (size_t)t.tiles_x * t.tiles_y * kToneLevels; }

// hist[tile][v] += the number of pixels with min(raw, 2^bits - 1) == v and raw inside `range` in each tile of the tiles_x x tiles_y
// grid over the width x height source (rows of pitch bytes; src and pitch even; tiles_x <= width, tiles_y <= height).  Exact for
// any content.  Ranged and plain: as launch_tone_hist.
hipError_t launch_clahe_hist(const ToneSetting &t, const uint8_t *src, int64_t pitch, int width, int height, const ValidRange &range,
                             uint32_t *hist, hipStream_t stream);

// luts[tile][i] = the tile's 8-bit value of min(i, 2^bits - 1) for all kToneLevels indices, counts[tile] = its pixels (the
// histogram's sum; 0, a tile with no valid pixel: SHIFT's table); hist is left all zero for the next frame.
hipError_t launch_clahe_tables(const ToneSetting &t, uint32_t *hist, uint8_t *luts, uint32_t *counts, hipStream_t stream);

// launch_gray16 under CLAHE: the blend of the four nearest tiles' tables per source pixel of the factor * width x factor * height
// source, then the rounded box average; with a mask, the validity mask as there.
hipError_t launch_clahe_gray16(const ToneSetting &t, const uint8_t *src, int64_t pitch, int factor, const uint8_t *luts, const ValidRange &range,
                               const uint8_t *frame_mask, uint8_t *gray, uint8_t *mask, int width, int height, hipStream_t stream);

}  // namespace nmi

namespace nmi_internal {

// 0 <= lo <= hi <= 65535 -> NMI_OK and *out; else NMI_ERR_INVALID_ARGUMENT, *out untouched.
int valid_range_check(int32_t lo, int32_t hi, nmi::ValidRange *out);

// *tm well formed for a context of width x height (include/nmi_hip.h; null: the default) -> NMI_OK and *out; else
// NMI_ERR_INVALID_ARGUMENT, *out untouched.
int tone_check(const nmi_tone_map *tm, int width, int height, nmi::ToneSetting *out);

// The device side of one tone setting's user (a context, a level, a stream): the histogram (zero between frames), the table
// with the window pair behind it, and which fixed setting the table currently holds; under CLAHE the tiles' histograms (zero
// between frames) and tables, up to 16 MiB and 4 MiB at 8 x 8 tiles of 16 bits.
struct ToneWork {
    nmi_mem::DeviceBuffer hist;  // uint32_t [kToneHistWords]
    nmi_mem::DeviceBuffer lut;   // uint8_t [kToneLevels], then int32_t [2]
    nmi_mem::DeviceBuffer tile_hist;  // CLAHE: clahe_hist_bytes
    nmi_mem::DeviceBuffer tile_luts;  // CLAHE: clahe_luts_bytes, then uint32_t [kClaheMaxTileCount]
    uint8_t *tile_tables() const { return tile_luts.as<uint8_t>(); }
    uint32_t *tile_counts(const nmi::ToneSetting &t) const { return reinterpret_cast<uint32_t *>(tile_luts.as<uint8_t>() + nmi::clahe_luts_bytes(t)); }
    // A deep source that is not GRAY16 (packed, big-endian, a 16-bit mosaic): its dense container, uint16_t [f H][f W], written by
    // nmi_unpack.h's kernel in front of every conversion and read by the GRAY16 kernels in the source's place.
    nmi_mem::DeviceBuffer container;
    bool built = false;          // lut holds the table of `fixed`
    nmi::ToneSetting fixed;
    uint8_t *table() const { return lut.as<uint8_t>(); }
    int32_t *window() const { return reinterpret_cast<int32_t *>(lut.as<uint8_t>() + nmi::kToneLevels); }
};

// Brings *w to what a GRAY16 conversion under t needs, on `stream`: the buffers (grown by nmi_mem.h's rule, the histogram
// cleared), and for SHIFT and WINDOW the table itself, built once per setting.  Not to be called inside a stream capture.
// container: the bytes of the source's container (container_bytes; 0 for GRAY16, which needs none), grown by the same rule.
hipError_t tone_prepare(ToneWork *w, const nmi::ToneSetting &t, hipStream_t stream, size_t container = 0);

// Bytes of the dense container of a factor * width x factor * height source in `format`: 2 per pixel for a deep format that
// unpacks (nmi_color.h's frame_needs_unpack), 0 for every other.
size_t container_bytes(int32_t format, int factor, int width, int height);

// The nodes in front of a GRAY16 conversion of the f W x f H source through one table: the histogram and the table for
// PERCENTILE and EQUALIZE, nothing otherwise.  Returns through *lut the table the conversion reads.  *w was prepared for t,
// which is not CLAHE.  The histogram counts the pixels inside `range`.
hipError_t launch_tone(const ToneWork &w, const nmi::ToneSetting &t, const nmi::ValidRange &range, const uint8_t *src, int64_t pitch,
                       int width, int height, const uint8_t **lut, hipStream_t stream);


// The CLAHE nodes in front of a conversion: the tile histograms of the width x height source, then the tile tables.
hipError_t launch_clahe_tone(const ToneWork &w, const nmi::ToneSetting &t, const nmi::ValidRange &range, const uint8_t *src, int64_t pitch,
                             int width, int height, hipStream_t stream);

// Every node of a GRAY16 conversion (nmi_gray_frame at factor 1, nmi_reduce_frame's, the intake's): the factor * width x factor *
// height source to the dense grey [height][width] under t -- launch_tone and launch_gray16, or CLAHE's three.  *w was prepared for t.
// The statistics are those of the pixels inside `range`.  mask_out (may be null): the conversion is the masked one and writes the
// validity mask, ANDed with frame_mask (dense [height][width], may be null, may be mask_out itself).
// format: NMI_FRAME_GRAY16, or a deep format that unpacks: then one more node in front, the unpack kernel (nmi_unpack.h) from
// src's rows of pitch bytes into w.container (prepared with container_bytes), which every node behind it reads as dense GRAY16.
hipError_t deep_gray(const ToneWork &w, const nmi::ToneSetting &t, const nmi::ValidRange &range, const uint8_t *src, int format, int64_t pitch,
                     int factor, const uint8_t *frame_mask, uint8_t *gray, uint8_t *mask_out, int width, int height, hipStream_t stream);

}  // namespace nmi_internal
