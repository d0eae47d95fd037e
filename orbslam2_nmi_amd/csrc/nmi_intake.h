// nmi_intake.h -- internal: a camera frame's way into a captured level or a stream (nmi_capi_pipeline.cpp).  The frame may be
// full-size (reduced to the search size), colour or pitched (converted to grey) and distorted (undistorted); FrameIntake is that
// setting as one value, and launch_intake the one place that knows which of the steps share a kernel.  Definitions:
// nmi_capi_intake.cpp.  The standalone calls (nmi_gray_frame, nmi_reduce_frame, nmi_undistort_frame) take explicit buffers and
// launch the same kernels themselves.
#pragma once
#include "nmi_hip.h"
#include "nmi_color.h"
#include "nmi_tone.h"
#include "nmi_undistort.h"

namespace nmi_internal {

struct FrameIntake {
    // Lens distortion (nmi_*_set_distortion, nmi_*_set_distortion_fisheye: one setting, the later call wins; ud.model tells the
    // two apart): the source (and its mask) are the raw frame, undistorted into gray_out (mask_out).
    bool distorted = false;
    nmi::UndistortParams ud{};
    // Frame format and reduction (nmi_*_set_frame_format, nmi_*_set_frame_reduction: one setting, the later call wins): the
    // source is frame_factor * H rows of frame_pitch bytes, each frame_factor * W pixels in frame_format.
    bool colored = false;                    // set: not a dense grey frame of the search size (always so with frame_factor > 1)
    int32_t frame_format = NMI_FRAME_GRAY;
    int64_t frame_pitch = 0;                 // row bytes (never 0 while colored)
    int32_t frame_factor = 1;
    // Tone map (nmi_*_set_tone_map): how a GRAY16 source's pixels become 8-bit; kept, and ignored, under every other format.
    nmi::ToneSetting tone;
    // Valid range (nmi_*_set_valid_range): which raw values of a deep source count in the tone map's statistics and are 1 in the
    // validity mask a masked or covered user asks launch_intake for; kept, and ignored, under every other format.
    nmi::ValidRange valid;

    bool reduced() const { return frame_factor > 1; }
    bool mosaic() const { return nmi::frame_is_bayer(frame_format); }
    bool deep() const { return nmi::frame_is_deep(frame_format); }  // GRAY16, or a format that unpacks to it
    bool validity() const { return deep() && valid.on(); }  // a masked or covered user's frame mask comes from the conversion
    // bytes of the container a deep source that is not GRAY16 is unpacked into (tone_prepare), 0 for every other format
    size_t container(int width, int height) const { return container_bytes(frame_format, frame_factor, width, height); }
    // grey frame first (into launch_intake's scratch), undistortion second: a reduction, a Bayer mosaic, whose taps would
    // each demosaic a 3 x 3 neighbourhood (profiles/sensor/README.md: the fused node takes twice the two nodes' time), and a
    // deep frame, whose table comes from the whole frame first
    bool two_nodes() const { return distorted && (reduced() || mosaic() || deep()); }
    bool own_frame() const { return distorted || colored; }  // the warps read gray_out, not the source
};

// dist == nullptr, or five zero coefficients: off.  A bad K or dist: NMI_ERR_INVALID_ARGUMENT, *in untouched.
int intake_set_distortion(FrameIntake *in, const double K[9], const float dist[5]);
// The fisheye form (K_raw == nullptr: K).  dist == nullptr: off; four zero coefficients stay on (an ideal equidistant lens).
int intake_set_distortion_fisheye(FrameIntake *in, const double K[9], const double K_raw[9], const float dist[4]);
// factor 1 .. 4, format and pitch checked on the full size factor * (width, height) (frame_format_check).  Dense grey of the search
// size: off (NMI_FRAME_GRAY, pitch 0).  A bad argument: NMI_ERR_INVALID_ARGUMENT, *in untouched.
int intake_set_frame(FrameIntake *in, int width, int height, int32_t factor, int32_t format, int64_t pitch);
// tm == nullptr: the default (SHIFT, 16 bits).  A bad *tm (CLAHE: for a context of width x height): NMI_ERR_INVALID_ARGUMENT, *in
// untouched.
int intake_set_tone_map(FrameIntake *in, int width, int height, const nmi_tone_map *tm);
// 0 <= lo <= hi <= 65535 (valid_range_check); (0, 65535): off.  A bad pair: NMI_ERR_INVALID_ARGUMENT, *in untouched.
int intake_set_valid_range(FrameIntake *in, int32_t lo, int32_t hi);

// Enqueues the intake's kernels: src (rows of src_row_bytes) -> the dense grey [H][W] gray_out; nothing when !in.own_frame().
//   reduced               launch_reduce, into scratch when distorted; then launch_undistort from scratch
//   mosaic, distorted     launch_gray into scratch; then launch_undistort from scratch
//   coloured, distorted   launch_undistort_color alone: each tap converted to grey, then the undistortion's arithmetic
//   distorted             launch_undistort
//   coloured              launch_gray
// A deep frame (GRAY16) takes deep_gray (nmi_tone.h) in launch_gray's and launch_reduce's place: launch_gray16 behind the histogram
// and table nodes of a PERCENTILE or EQUALIZE tone map, or CLAHE's tile histograms, tile tables and blending conversion; tone is
// its prepared work area (tone_prepare), unused for every other format.  A deep format that is not GRAY16 (packed, big-endian,
// a 16-bit mosaic) has one more node in front of those, on the same chain: the unpack kernel into tone's container.  The
// statistics are those of the pixels inside in.valid.
// mask_out (may be null; only written when distorted) = the undistorted src_mask (dense [H][W], may be null: border only).
// valid_out (may be null; only a deep frame writes it; given by a masked or covered user while in.validity()): "the validity mask
// goes here" -- the same conversion node, as its masked instantiation, writes nmi_deep_frame's d_mask there: validity ANDed with
// src_mask (dense [H][W], may be null, may be valid_out itself).  Not distorted, it is the frame mask the warp masks are made
// from; distorted, the undistortion node's raw mask in src_mask's place.
// scratch is [H][W] and needed only when in.two_nodes().
hipError_t launch_intake(const FrameIntake &in, const ToneWork &tone, const uint8_t *src, int64_t src_row_bytes, const uint8_t *src_mask,
                         uint8_t *scratch, uint8_t *gray_out, uint8_t *mask_out, uint8_t *valid_out, int width, int height,
                         hipStream_t stream);

}  // namespace nmi_internal
