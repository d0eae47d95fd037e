// nmi_capi_intake.cpp -- the frame intake the captured levels and the streams share (nmi_intake.h): its settings, checked
// and normalised, and its kernel launches.
#include "nmi_intake.h"

#include "nmi_color.h"
#include "nmi_reduce.h"

namespace nmi_internal {

int intake_set_distortion(FrameIntake *in, const double K[9], const float dist[5])
{
    nmi::UndistortParams ud{};
    bool identity = true;
    if (dist && undistort_params(K, dist, &ud, &identity) != NMI_OK) return NMI_ERR_INVALID_ARGUMENT;
    in->distorted = dist && !identity;  // five zero coefficients: as never distorted
    in->ud = ud;
    return NMI_OK;
}

int intake_set_distortion_fisheye(FrameIntake *in, const double K[9], const double K_raw[9], const float dist[4])
{
    nmi::UndistortParams ud{};
    if (dist && fisheye_params(K, K_raw, dist, &ud) != NMI_OK) return NMI_ERR_INVALID_ARGUMENT;
    in->distorted = dist != nullptr;  // no identity case: zero coefficients are an ideal equidistant lens, still a remap
    in->ud = ud;
    return NMI_OK;
}

int intake_set_frame(FrameIntake *in, int width, int height, int32_t factor, int32_t format, int64_t pitch)
{
    FrameSource full;  // (no frame yet: its base is checked where it is set)
    if (frame_source_check(format, pitch, factor, width, height, nullptr, &full) != NMI_OK) return NMI_ERR_INVALID_ARGUMENT;
    const bool on = !full.identity || factor > 1;  // dense grey of the search size: as never formatted
    in->colored = on;
    in->frame_format = on ? format : NMI_FRAME_GRAY;
    in->frame_pitch = on ? full.row_bytes : 0;
    in->frame_factor = factor;
    return NMI_OK;
}

int intake_set_tone_map(FrameIntake *in, int width, int height, const nmi_tone_map *tm) { return tone_check(tm, width, height, &in->tone); }

int intake_set_valid_range(FrameIntake *in, int32_t lo, int32_t hi) { return valid_range_check(lo, hi, &in->valid); }

hipError_t launch_intake(const FrameIntake &in, const ToneWork &tone, const uint8_t *src, int64_t src_row_bytes, const uint8_t *src_mask,
                         uint8_t *scratch, uint8_t *gray_out, uint8_t *mask_out, uint8_t *valid_out, int width, int height,
                         hipStream_t stream)
{
    const uint8_t *raw_mask = mask_out ? src_mask : nullptr;
    if (in.deep()) {  // (distorted: two_nodes())
        // the tone tables of the full-size source where they come from the frame, then the conversion (and reduction); with
        // valid_out the masked conversion, whose validity mask takes src_mask's place from here on
        const hipError_t e = deep_gray(tone, in.tone, in.valid, src, in.frame_format, src_row_bytes, in.frame_factor,
                                       valid_out ? src_mask : nullptr, in.distorted ? scratch : gray_out, valid_out, width, height, stream);
        if (e != hipSuccess || !in.distorted) return e;
        if (valid_out && mask_out) raw_mask = valid_out;
        return nmi::launch_undistort(in.ud, scratch, raw_mask, gray_out, mask_out, width, height, stream);
    }
    if (in.reduced()) {  // one node converts and reduces; distorted: the undistortion node reads the reduced frame
        const hipError_t e = nmi::launch_reduce(src, in.frame_format, src_row_bytes, in.frame_factor, in.distorted ? scratch : gray_out, width,
                                                height, stream);
        if (e != hipSuccess || !in.distorted) return e;
        return nmi::launch_undistort(in.ud, scratch, raw_mask, gray_out, mask_out, width, height, stream);
    }
    if (in.two_nodes()) {  // a mosaic: demosaiced to grey once, not at every tap
        const hipError_t e = nmi::launch_gray(src, in.frame_format, src_row_bytes, scratch, width, height, stream);
        return e != hipSuccess ? e : nmi::launch_undistort(in.ud, scratch, raw_mask, gray_out, mask_out, width, height, stream);
    }
    if (in.distorted && in.colored)
        return nmi::launch_undistort_color(in.ud, src, in.frame_format, src_row_bytes, raw_mask, gray_out, mask_out, width, height, stream);
    if (in.distorted) return nmi::launch_undistort(in.ud, src, raw_mask, gray_out, mask_out, width, height, stream);
    if (in.colored) return nmi::launch_gray(src, in.frame_format, src_row_bytes, gray_out, width, height, stream);
    return hipSuccess;
}

}  // namespace nmi_internal
