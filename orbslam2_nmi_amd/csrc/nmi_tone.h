// nmi_tone.h -- internal interface of the deep grey frames (NMI_FRAME_GRAY16, include/nmi_hip.h): the tone map as a checked
// value, the device buffers that go with it, and the kernels of nmi_tone.hip.  Every mode goes through one uint8 [65536] table:
// the fixed modes' (SHIFT, WINDOW) is built when the setting changes, the data-dependent ones' (PERCENTILE, EQUALIZE) by two
// kernels in front of every conversion, and TABLE's is the caller's.  Used by nmi_capi_tone.cpp (the entries), nmi_capi_color.cpp,
// nmi_capi_reduce.cpp and nmi_capi_intake.cpp (levels and streams).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

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
    int32_t plateau = 0;             // EQUALIZE
    const uint8_t *d_lut = nullptr;  // TABLE: the caller's
    bool from_frame() const { return mode == NMI_TONE_PERCENTILE || mode == NMI_TONE_EQUALIZE; }
    bool operator==(const ToneSetting &o) const
    {
        return mode == o.mode && bits == o.bits && lo == o.lo && hi == o.hi && p_lo == o.p_lo && p_hi == o.p_hi && plateau == o.plateau &&
               d_lut == o.d_lut;
    }
};

// hist[v] += the number of pixels with min(raw, 2^bits - 1) == v among the height rows of pitch bytes at src, each width
// little-endian 16-bit pixels (src and pitch even).  Exact for any content; hist is uint32 [kToneLevels].
hipError_t launch_tone_hist(const uint8_t *src, int64_t pitch, int width, int height, int bits, uint32_t *hist, hipStream_t stream);

// lut[i] = the setting's 8-bit value of min(i, 2^bits - 1) for all kToneLevels indices, and window[0 .. 1] = the {lo, hi} pair
// nmi_tone_lut reports (window may be null).  hist: for a from_frame() mode the frame's histogram at the head of a buffer of
// kToneHistWords words, left all zero for the next frame (two kernels); never read otherwise (one kernel).
hipError_t launch_tone_table(const ToneSetting &t, uint32_t *hist, uint8_t *lut, int32_t *window, hipStream_t stream);

// nmi_gray_frame (factor 1) and nmi_reduce_frame (factor 2 .. 4) of a GRAY16 source of factor * height rows of pitch bytes,
// each factor * width pixels: lut[min(raw, 2^bits - 1)] per source pixel, then the rounded box average (nmi_reduce_device.h).
// lut is the table of launch_tone_table, or a TABLE setting's own.
hipError_t launch_gray16(const uint8_t *src, int64_t pitch, int factor, const uint8_t *lut, int bits, uint8_t *gray, int width, int height,
                         hipStream_t stream);

}  // namespace nmi

namespace nmi_internal {

// *tm well formed (include/nmi_hip.h; null: the default) -> NMI_OK and *out; else NMI_ERR_INVALID_ARGUMENT, *out untouched.
int tone_check(const nmi_tone_map *tm, nmi::ToneSetting *out);

// The device side of one tone setting's user (a context, a level, a stream): the histogram (zero between frames), the table
// with the window pair behind it, and which fixed setting the table currently holds.
struct ToneWork {
    nmi_mem::DeviceBuffer hist;  // uint32_t [kToneHistWords]
    nmi_mem::DeviceBuffer lut;   // uint8_t [kToneLevels], then int32_t [2]
    bool built = false;          // lut holds the table of `fixed`
    nmi::ToneSetting fixed;
    uint8_t *table() const { return lut.as<uint8_t>(); }
    int32_t *window() const { return reinterpret_cast<int32_t *>(lut.as<uint8_t>() + nmi::kToneLevels); }
};

// Brings *w to what a GRAY16 conversion under t needs, on `stream`: the buffers (grown by nmi_mem.h's rule, the histogram
// cleared), and for SHIFT and WINDOW the table itself, built once per setting.  Not to be called inside a stream capture.
hipError_t tone_prepare(ToneWork *w, const nmi::ToneSetting &t, hipStream_t stream);

// The nodes in front of a GRAY16 conversion of the f W x f H source: the histogram and the table for a from_frame() mode,
// nothing otherwise.  Returns through *lut the table the conversion reads.  *w was prepared for t.
hipError_t launch_tone(const ToneWork &w, const nmi::ToneSetting &t, const uint8_t *src, int64_t pitch, int width, int height,
                       const uint8_t **lut, hipStream_t stream);

}  // namespace nmi_internal
