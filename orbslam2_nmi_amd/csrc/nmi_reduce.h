// nmi_reduce.h -- internal interface of the full-size camera frames (nmi_reduce.hip), used by nmi_capi_reduce.cpp
// (nmi_reduce_frame) and by the captured levels and streams of nmi_capi_pipeline.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nmi {

// gray[y][x] = the rounded box average (include/nmi_hip.h, nmi_reduce_frame) of the factor x factor grey values
// (nmi_gray_frame's rule) of source pixels (factor * x .., factor * y ..) of the factor * height rows of pitch bytes at src in
// format (an NMI_FRAME_* value; pitch > 0, the rows' bytes).  factor is 2, 3 or 4 (1 is launch_gray).  gray is dense
// [height][width] and does not overlap the source.
hipError_t launch_reduce(const uint8_t *src, int format, int64_t pitch, int factor, uint8_t *gray, int width, int height, hipStream_t stream);

// mask[y][x] = 1 where all factor x factor bytes of the dense [factor * height][factor * width] src_mask are nonzero, else 0.
// factor is 1 .. 4.
hipError_t launch_reduce_mask(const uint8_t *src_mask, int factor, uint8_t *mask, int width, int height, hipStream_t stream);

}  // namespace nmi
