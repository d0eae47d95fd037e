// nmi_unpack.h -- internal interface of the deep raw formats (include/nmi_hip.h "Deep frames": NMI_FRAME_GRAY16_BE, MONO10P,
// MONO12P, RAW10, RAW12, BAYER16_*): one kernel family (nmi_unpack.hip) that writes the dense GRAY16 container every deep kernel
// of nmi_tone.h reads.  Used by nmi_capi_tone.cpp: deep_gray (every conversion) and nmi_unpack_frame.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nmi_hip.h"

namespace nmi {

// gray16[y][x] = the container pixel u(x, y) of the height rows of pitch bytes at src, each width pixels in format (one of the
// nine that nmi_color.h's frame_needs_unpack names; width whole groups, pitch >= the row's bytes; the 2-byte formats' src and
// pitch even, a BAYER16 mosaic at least 2 x 2).  gray16 is dense [height][width], 2-byte aligned, and does not overlap the
// source.  No byte past a row's last is read.
hipError_t launch_unpack(const uint8_t *src, int format, int64_t pitch, uint16_t *gray16, int width, int height, hipStream_t stream);

}  // namespace nmi
