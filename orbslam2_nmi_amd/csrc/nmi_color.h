// nmi_color.h -- internal interface of the colour and pitched camera frames (nmi_color.hip, and the colour instantiation of the
// undistortion kernel in nmi_undistort.hip), used by nmi_capi_color.cpp (nmi_gray_frame) and by the captured levels and streams
// of nmi_capi_pipeline.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nmi_hip.h"
#include "nmi_undistort.h"

namespace nmi {

// gray[y][x] = the grey value (include/nmi_hip.h, nmi_gray_frame) of pixel (x, y) of the height rows of pitch bytes at src in
// format (an NMI_FRAME_* value; pitch > 0, the rows' bytes).  gray is dense [height][width] and does not overlap the source.
hipError_t launch_gray(const uint8_t *src, int format, int64_t pitch, uint8_t *gray, int width, int height, hipStream_t stream);

// format is one of NMI_FRAME_BAYER_*.
inline bool frame_is_bayer(int format) { return format >= NMI_FRAME_BAYER_RGGB && format <= NMI_FRAME_BAYER_BGGR; }

// (NMI_FRAME_GRAY16 is not launch_gray's or launch_reduce's: it needs its tone table, nmi_tone.h's launch_gray16.)

// The deep raw formats (include/nmi_hip.h "Deep frames"): format is one of NMI_FRAME_BAYER16_*; a deep source that is not its
// own container and goes through nmi_unpack.h's kernel first; any deep source, GRAY16 included; a deep source of 2-byte words
// (even base, even pitch), as against the byte-packed ones.
inline bool frame_is_bayer16(int format) { return format >= NMI_FRAME_BAYER16_RGGB && format <= NMI_FRAME_BAYER16_BGGR; }
inline bool frame_needs_unpack(int format) { return format == NMI_FRAME_GRAY16_BE || (format >= NMI_FRAME_MONO10P && format <= NMI_FRAME_BAYER16_BGGR); }
inline bool frame_is_deep(int format) { return format == NMI_FRAME_GRAY16 || frame_needs_unpack(format); }
inline bool frame_is_words(int format) { return format == NMI_FRAME_GRAY16 || format == NMI_FRAME_GRAY16_BE || frame_is_bayer16(format); }

// launch_gray (factor 1) and launch_reduce (nmi_reduce.h; factor 2 .. 4) of a Bayer mosaic of factor * height rows of factor *
// width bytes (both >= 2), in one kernel (nmi_bayer.hip): launch_gray and launch_reduce pass their Bayer formats on to it.
hipError_t launch_bayer(const uint8_t *src, int format, int64_t pitch, int factor, uint8_t *gray, int width, int height, hipStream_t stream);

// launch_undistort on the grey values of a colour, pitched or packed-YUV raw frame (not a Bayer mosaic), in one kernel: equal to
// launch_gray into a dense frame followed by launch_undistort on it.  raw_mask and frame_mask are dense [height][width], as there.
hipError_t launch_undistort_color(const UndistortParams &p, const uint8_t *src, int format, int64_t pitch, const uint8_t *raw_mask,
                                  uint8_t *frame, uint8_t *frame_mask, int width, int height, hipStream_t stream);

}  // namespace nmi

namespace nmi_internal {

// Bytes per pixel of an NMI_FRAME_* format, 0 for an unknown one and for the byte-packed ones (10 and 12 bits per pixel).
int frame_bytes_per_pixel(int32_t format);

// Dense bytes of a row of width pixels in an NMI_FRAME_* format (nmi_frame_row_bytes): 0 for an unknown format, a width <= 0
// or one that is not whole groups (4 pixels in 5 bytes, 2 in 3).
int64_t frame_row_bytes(int32_t format, int64_t width);

// The source's first byte is aligned as format asks: the 2-byte deep formats on 2 bytes, every other format anywhere.
inline bool frame_base_ok(int32_t format, const void *src) { return !nmi::frame_is_words(format) || ((uintptr_t)src % 2) == 0; }

// format known, width whole groups, pitch 0 (dense) or >= the row's bytes, a Bayer mosaic (8 or 16 bits) at least 2 x 2, a
// 2-byte deep format's pitch even (and a deep frame below 2^32 pixels: its histogram counts in 32 bits) -> NMI_OK, *row_bytes =
// the rows' pitch (frame_row_bytes for 0) and *identity = the frame is dense grey (GRAY with pitch 0 or width: no conversion);
// else NMI_ERR_INVALID_ARGUMENT.  width and height are the source's.
int frame_format_check(int32_t format, int64_t pitch, int width, int height, int64_t *row_bytes, bool *identity);

// The bytes [lo, hi) of a device buffer; lo == hi: nothing, which is what a NULL buffer comes to.  Two buffers an entry may not
// see overlap `meet`; nothing meets nothing.
struct Span {
    uintptr_t lo, hi;
};
inline Span span_of(const void *p, size_t bytes) { return {(uintptr_t)p, (uintptr_t)p + (p ? bytes : 0)}; }
inline bool meet(const Span &a, const Span &b) { return a.lo < a.hi && b.lo < b.hi && a.lo < b.hi && b.lo < a.hi; }

// The full-size source of an entry that converts factor * width x factor * height pixels at d_src to width x height.
struct FrameSource {
    int width = 0, height = 0;  // the full size
    int64_t row_bytes = 0;      // the rows' pitch (frame_format_check's)
    bool identity = false;      // frame_format_check's
    Span bytes{0, 0};           // from d_src to the end of its last row's pixels; nothing for a NULL d_src
};

// factor 1 .. 4, the full size fits int, frame_format_check on it, and d_src aligned as format asks (frame_base_ok; NULL, a
// setting checked ahead of its frames, passes) -> NMI_OK and *out; else NMI_ERR_INVALID_ARGUMENT, *out untouched.
int frame_source_check(int32_t format, int64_t pitch, int32_t factor, int width, int height, const void *d_src, FrameSource *out);

}  // namespace nmi_internal
