/*
 * nmi_hip.h -- C ABI of libnmi_hip.so: MI355X (gfx950) implementation of the NMI pose-candidate
 * scoring path of gsanya/orbslam2_NMI.
 *
 * This is the drop-in boundary.  Each entry point names the reference interface it replaces
 * (paths relative to the reference repository root).  Plain pointers and sizes only; no C++,
 * torch or OpenCV types.  All image pointers are DEVICE pointers unless a name starts with h_.
 * Every function returns NMI_OK (0) or a negative error code; nothing calls exit() (the
 * reference aborts the process through checkCudaErrors, Thirdparty/CUDA_Functions/kernel.cu:53-113).
 *
 * Data conventions:
 *   image           uint8 [height][width], contiguous, row stride = width
 *                   (cv::cuda::createContinuous CV_8UC1, Thirdparty/Localization/image.cpp:67).
 *                   The camera frame alone may also come in colour, as a Bayer mosaic, as packed YUV or with a row stride: nmi_gray_frame,
 *                   nmi_level_set_frame_format, nmi_stream_set_frame_format (NMI_FRAME_*); and at 2, 3 or 4 times the
 *                   context's size: nmi_reduce_frame, nmi_level_set_frame_reduction, nmi_stream_set_frame_reduction.
 *   render          same shape; stored bottom-up when nmi_params.render_bottom_up = 1, which is how
 *                   the reference samples the GL texture (NMI.cu:82).
 *   render_stack    uint8 [S][height][width],  s = (sZ*nSy + sY)*nSx + sX
 *   warp_stack      uint8 [Wn][height][width], w = (wZ*nWy + wY)*nWx + wX
 *   ratings         float [Wn][S]; ratings[w*S + s] == rating[wZ][wY][wX][sZ][sY][sX]
 *                   (Thirdparty/Localization/localization.hpp:36, src/Tracking.cc:1892).
 *   linear index    w*S + s -- the order helperFunctions::find_max_elements scans
 *                   (Thirdparty/Localization/helperFunctions.cpp:53-64).
 */
#ifndef NMI_HIP_H
#define NMI_HIP_H

#include <stddef.h>
#include <stdint.h>

#include "nmi_refined_peak.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NMI_HIP_ABI_VERSION 2 /* 2 (round 4): + nmi_pix_status, NMI_OPT_SPLIT 1; round 3 had added nmi_split_status,
                                 nmi_level_create_block, nmi_level_create_mesh_block, nmi_level_run_rccl, nmi_stream_submit_block and
                                 changed NMI_OPT_TILE_QUEUE from queue items to entries per tile bin without a bump; still 2 after
                                 the purely additive nmi_warp_stack_masked, nmi_search_grid_masked, nmi_last_mask_counts,
                                 nmi_level_set_masks, nmi_level_copy_masks, after nmi_level_set_coverage,
                                 nmi_level_copy_coverage, and after nmi_pack_mask_bits, nmi_stream_submit_masked,
                                 nmi_stream_submit_masked_block, nmi_stream_submit_covered, nmi_stream_submit_covered_block,
                                 nmi_stream_copy_counts, and after nmi_undistort_frame,
                                 nmi_level_set_distortion, nmi_stream_set_distortion, and after nmi_gray_frame,
                                 nmi_level_set_frame_format, nmi_stream_set_frame_format, and after nmi_reduce_frame,
                                 nmi_level_set_frame_reduction, nmi_stream_set_frame_reduction, and after
                                 nmi_undistort_frame_fisheye, nmi_level_set_distortion_fisheye,
                                 nmi_stream_set_distortion_fisheye, and after nmi_level_set_valid_range,
                                 nmi_stream_set_valid_range, and after nmi_refine_peaks, nmi_level_set_refine,
                                 nmi_level_copy_refined */

/* Error codes.  HIP errors are reported as NMI_ERR_HIP - (int)hipError_t, RCCL as NMI_ERR_RCCL - (int)ncclResult_t. */
#define NMI_OK 0
#define NMI_ERR_INVALID_ARGUMENT (-1)
#define NMI_ERR_UNSUPPORTED (-2)
#define NMI_ERR_NO_DEVICE (-3)
#define NMI_ERR_NOT_READY (-4)
#define NMI_ERR_HIP (-1000)
#define NMI_ERR_RCCL (-2000)

/* Score selector; values follow the reference's macros ENMI 0 / SUC 1 (Thirdparty/CUDA_Functions/kernel.cuh:22-23).
 * The reference ignores its run-time NMI_mode argument (kernel.cu:49) and compiles SUC in (NMI.cu:344,352). */
#define NMI_MODE_ENMI 0
#define NMI_MODE_SUC 1

typedef struct nmi_ctx nmi_ctx;

/*
 * Behaviour switches that are compile-time macros in the reference, as run-time fields whose
 * defaults (nmi_params_default) equal the reference's values.
 */
typedef struct nmi_params {
    int32_t width;            /* Camera.Width  / kernel.cu:49 'width'  */
    int32_t height;           /* Camera.Height / kernel.cu:49 'height' */
    int32_t bins;             /* 256 = HISTOGRAM256_BIN_COUNT (NMI.cuh:39); 128/64/32/16 use intensity >> k */
    int32_t mode;             /* NMI_MODE_SUC (kernel.cuh:23) or NMI_MODE_ENMI (kernel.cuh:22) */
    int32_t use_bg;           /* nmi_prop_BG (Thirdparty/Localization/allProperties.hpp:38); default 1 */
    int32_t render_bottom_up; /* 1 = vertical flip of the render as in NMI.cu:82; default 1 */
    int32_t device;           /* HIP device ordinal; -1 = the calling thread's current device */
    int32_t max_candidates;   /* ignored (kept for ABI compatibility): rating tables are caller-owned */
    void *stream;             /* hipStream_t to run on; NULL = the context creates its own */
    int32_t reserved[8];      /* must be 0 */
} nmi_params;

/* Fills *p with the reference defaults: bins 256, SUC, BG on, bottom-up render, current device. */
int nmi_params_default(nmi_params *p, int32_t width, int32_t height);

/*
 * Persistent workspace.  Replaces the per-call allocations of CUDAF::NMIWithCuda_noMask
 * (7 cudaMalloc kernel.cu:67-73, initHistogram256all NMI.cu:171-177, the frees at kernel.cu:103-109
 * and closeHistogram256all NMI.cu:180-185) and the file-static buffers NMI.cu:165-167.
 * One context = one stream; not thread-safe across threads (the reference is called from the
 * Tracking thread only, src/Tracking.cc:1886).  Several contexts may search at the same time from several threads; if they
 * score SMALL grids (up to 64 candidates) concurrently, give each a share of the device with NMI_OPT_WORKGROUPS
 * (e.g. compute units / number of contexts): the split kernel used for small grids wants all workgroups of a launch
 * resident at once, and two such launches that together exceed the device (or a neighbour -- another process, a GL or
 * compute client of the same GPU -- holding compute units) make each other wait until a 2 ms guard ends the wait.  The
 * search of THAT launch is then redone by the one-workgroup-per-candidate kernel (correct results, one slow call) and the
 * split forms pause for the next 16 small-grid launches of the context -- 32, 64, ... 4096 when the retry times out again --
 * after which they are used again; nmi_split_status reports the state.  Calls that only enqueue (h_key == NULL) never use
 * the split kernel: nobody would look for its timeout.
 */
int nmi_create(const nmi_params *params, nmi_ctx **out_ctx);
int nmi_destroy(nmi_ctx *ctx);

/* Run subsequent work on this hipStream_t (not owned).  NULL restores the context's own stream. */
int nmi_set_stream(nmi_ctx *ctx, void *stream);
/* Blocks until everything enqueued on the context's stream has finished. */
int nmi_synchronize(nmi_ctx *ctx);

/*
 * One candidate: replaces CUDAF::NMIWithCuda_noMask (Thirdparty/CUDA_Functions/kernel.cuh:37,
 * kernel.cu:49-114) with the render given as a linear device buffer instead of a GL texture name.
 * Blocking; *h_score receives the value the reference copies back at kernel.cu:100.
 */
int nmi_eval_pair(nmi_ctx *ctx, const uint8_t *render, const uint8_t *warped, float *h_score);

/*
 * A batch of independent candidates, each a (render, warped frame) pair of device images: the scores the reference would
 * get from n consecutive calls of CUDAF::NMIWithCuda_noMask (kernel.cu:49-114), e.g. the Wn warps of the inner loop at
 * src/Tracking.cc:1883-1894 against the render of the current outer iteration.  h_renders / h_warps are HOST arrays of n
 * device pointers (the same pointer may appear many times); h_scores receives n floats.  Blocking.  One launch scores up
 * to compute_units / 4 pairs (several workgroups per pair), larger batches take several launches.
 */
int nmi_eval_pairs(nmi_ctx *ctx, const uint8_t *const *h_renders, const uint8_t *const *h_warps, int32_t n, float *h_scores);

/*
 * Same evaluation, additionally exporting the exact integer histograms and the three entropy sums
 * (the intermediate buffers d_JointHistogram / d_Histogram1 / d_Histogram2 and element 0 of
 * d_Entropy1 / d_Entropy2 / d_JointEntropyShort before the score is formed, kernel.cu:59-95).
 * Any of the device output pointers may be NULL.  joint is [256][256] indexed [render][warped].
 */
int nmi_eval_pair_debug(nmi_ctx *ctx, const uint8_t *render, const uint8_t *warped, float *h_score,
                        uint32_t *d_joint /*[65536]*/, uint32_t *d_hist_render /*[256]*/,
                        uint32_t *d_hist_warped /*[256]*/, float *d_sums /*[3]: A1, A2, A3*/);

/*
 * Whole candidate grid + best-pose pick: replaces the 6-nested loop of Tracking::RelocalizeWithNMI
 * (src/Tracking.cc:1879-1902: S renders x Wn warps calls of NMIWithCuda_noMask) and
 * helperFunctions::find_max_elements + the caller's [0] pick (helperFunctions.cpp:50-103,
 * Tracking.cc:1905,1952-1953).
 *   d_ratings       device float [Wn*S], or NULL when only the winner is wanted (no rating table is stored then).
 *   h_best_index    linear index w*S + s of the winner: max starts at 0, strict '>', lowest index
 *                   among cells equal to the max; -1 if no cell qualifies (every score negative or
 *                   NaN, where the reference indexes an empty vector).
 *   h_best_score    the winner's score.
 * Blocking (8-byte read-back of the packed winner).  With the default result path the call returns when the kernel's
 * last workgroup has posted the winner to pinned host memory; when d_ratings is given it additionally waits for the
 * context's stream, so the table is complete and visible to every stream when the call returns.
 */
int nmi_search_grid(nmi_ctx *ctx, const uint8_t *render_stack, int32_t S, const uint8_t *warp_stack, int32_t Wn,
                    float *d_ratings, int64_t *h_best_index, float *h_best_score);

/*
 * Sharded form for one rank of a multi-GPU search (new; the reference is single-GPU).
 * This rank holds renders [s_offset, s_offset + S_local) of a global grid with S_total renders and
 * the full warp stack.  The kernel writes the rank's best candidate as a packed key to *d_key
 * (device uint64, may be NULL to use an internal slot) and, if h_key != NULL, blocks and copies it
 * to the host.  key = float_bits(score) << 32 | (0xFFFFFFFF - global_linear_index) for score >= 0
 * and 0 for "no candidate"; the maximum over ranks (uint64 or int64 MAX all-reduce) is the global
 * winner with the reference's lowest-index tie-break.  d_ratings (nullable) is [Wn][S_local].
 * With h_key == NULL the call only enqueues work on the context's stream.
 */
int nmi_search_grid_shard(nmi_ctx *ctx, const uint8_t *render_stack, int32_t S_local, int32_t s_offset,
                          int32_t S_total, const uint8_t *warp_stack, int32_t Wn, float *d_ratings,
                          uint64_t *d_key, uint64_t *h_key);

/*
 * The same for any rectangular block of the grid: renders [s_offset, s_offset + S_local) x warps [w_offset, w_offset +
 * Wn_local) of an S_total x Wn_total grid (used when there are fewer renders than ranks and the warp axis is sharded
 * instead).  d_ratings (nullable) is [Wn_local][S_local]; the key carries the global linear index w * S_total + s.
 */
int nmi_search_grid_block(nmi_ctx *ctx, const uint8_t *render_stack, int32_t S_local, int32_t s_offset, int32_t S_total,
                          const uint8_t *warp_stack, int32_t Wn_local, int32_t w_offset, int32_t Wn_total, float *d_ratings,
                          uint64_t *d_key, uint64_t *h_key);

/*
 * Warp-stack producer: replaces Image::calculateWarping (Thirdparty/Localization/image.cpp:115-128),
 * i.e. Wn calls of cv::cuda::warpPerspective(frame, warped[w], M[w], size) with INTER_LINEAR / BORDER_CONSTANT 0.
 *   h_forward   host doubles [Wn][9], row-major 3x3 forward homographies K*R*K^-1 exactly as image.cpp:106 stores them
 *               (nmi_warp_homographies builds them from K and the warp axes of a grid);
 *   d_frame     device uint8 [H][W]; d_warp_stack device uint8 [Wn][H][W], w = (wZ*nWy + wY)*nWx + wX.
 * Enqueued on the context's stream (no synchronisation).  OpenCV is not part of the reference tree: parity of the
 * interpolation arithmetic is unpinned (see the kernel comment).
 * A matrix with a non-finite entry, or singular (det == 0 after it is scaled to a largest |entry| in [1, 2)), makes the
 * call return NMI_ERR_INVALID_ARGUMENT before anything is enqueued.  Any other scale is accepted: M and c M (c != 0)
 * give the same warp, and for c a power of two the same bytes.  The same rule holds for nmi_warp_stack_masked,
 * nmi_level_run and nmi_level_run_rccl (a rejected level run leaves the level as it was).
 */
int nmi_warp_homographies(const double K[9], const int32_t num_warp_xyz[3], const float step_rad_xyz[3],
                          double *h_forward /*[Wn][9]*/);
int nmi_warp_stack(nmi_ctx *ctx, const uint8_t *d_frame, const double *h_forward, int32_t Wn, uint8_t *d_warp_stack);

/*
 * Masked search: which pixels of the camera frame take part in the score.  The reference's entry point is
 * CUDAF::NMIWithCuda_noMask (Thirdparty/CUDA_Functions/kernel.cuh:35-37, under "no masks:"); these are its masked siblings
 * for the whole grid (new).
 *
 * A warp mask is uint8 [Wn][H][W] in the coordinates of the warp stack (top-down rows of the camera frame); nonzero = the
 * pixel takes part, 0 = excluded.  For candidate (warp w, render s) pixel pos enters the joint histogram iff
 *   mask[w][pos] != 0, and the background rule passes (use_bg = 0: both RAW intensities nonzero, before the >> shift);
 * its render pixel is the one nmi_search_grid pairs with it (flipped when render_bottom_up).  len_w = popcount(mask[w])
 * replaces W*H in the per-bin term fl32(p * fl32(log2(p))), p = fl32(c / len_w); like W*H it is not reduced by the
 * background rule.  Trees, SUC / ENMI, the all-zero guard, the rating layout [Wn][S] and the arg-max rule are those of
 * nmi_search_grid, so an all-ones mask gives nmi_search_grid's bits, and an empty mask (len_w = 0) scores 0.0 for every
 * render of its warp.
 *
 * nmi_warp_stack_masked: nmi_warp_stack (the warp stack is byte-identical) plus the masks of the warps.  Pixel (x, y) of
 * warp w is valid (1, else 0) when its fp32 source coordinate (xs, ys) -- computed as the warp computes it -- passes the
 * warp's source test -2 < xs < W+1, -2 < ys < H+1, when every bilinear tap with nonzero weight lies inside the frame
 * (x1 = floor(xs) >= 0, x1 + (xs != x1) <= W-1, the same for rows), and, given d_frame_mask (uint8 [H][W], nullable = all
 * valid), when every such tap is nonzero in it.  The identity homography gives an all-ones mask and warp == frame.
 * Enqueued on the context's stream, like nmi_warp_stack; non-finite or singular matrices are rejected as there.
 *
 * nmi_search_grid_masked: nmi_search_grid with the masks; len_w is counted on the device from warp_masks (the source of
 * truth: the masks need not come from nmi_warp_stack_masked).  A NULL warp_masks is NMI_ERR_INVALID_ARGUMENT.  Blocking
 * exactly like nmi_search_grid.  NMI_OPT_SPLIT* choose the kernel, never the result: mid-size grids take the masked
 * pixel-range kernel where plan_search's rules for nmi_search_grid pick pixel ranges (NMI_OPT_SPLIT 0 keeps the masked grid
 * kernel, NMI_OPT_SPLIT 1 + NMI_OPT_SPLIT_PIXELS P forces P ranges wherever they fit); NMI_OPT_CONTENT_PATH does not apply.
 *
 * nmi_last_mask_counts: len_w of the latest masked search's first n warps (n <= its Wn) to host memory.  Blocking.
 *
 * Render-side masks: see nmi_search_grid_covered below.  Captured levels: nmi_level_set_masks.  Streams:
 * nmi_stream_submit_masked.  Not masked (yet): shard / block / RCCL forms of the standalone search, the CUDAF shim.
 */
int nmi_warp_stack_masked(nmi_ctx *ctx, const uint8_t *d_frame, const uint8_t *d_frame_mask /* nullable: all valid */,
                          const double *h_forward, int32_t Wn, uint8_t *d_warp_stack, uint8_t *d_warp_masks);
int nmi_search_grid_masked(nmi_ctx *ctx, const uint8_t *render_stack, int32_t S, const uint8_t *warp_stack,
                           const uint8_t *warp_masks, int32_t Wn, float *ratings /* nullable */,
                           int64_t *best_linear_idx, float *best_score);
int nmi_last_mask_counts(nmi_ctx *ctx, int32_t *h_counts, int32_t n);

/*
 * Covered search: masks on both sides.  The map side's mask is the coverage of a render: both renderers clear to 255
 * (glClearColor(1,1,1), rendering.hpp:533) and the background rule drops only raw zeros, so without it every pixel the map
 * does not cover enters the joint histogram as a solid 255.
 *
 * A render mask is uint8 [S][H][W] in the render's own layout (bottom-up rows, like the render stack); nonzero = covered.
 * Candidate (warp w, render s) counts pixel pos of the warp iff
 *   warp_masks[w][pos] != 0, render_masks[s][rpos] != 0 (rpos: the render pixel nmi_search_grid pairs with pos, row-flipped
 *   when render_bottom_up), and the background rule passes on the raw intensities.
 * len[w][s] = the number of pos where both masks are nonzero (like W*H, not reduced by the background rule) replaces W*H in
 * the term fl32(p * fl32(log2_f64(p))), p = fl32(c / len[w][s]); len = 0 scores 0.0.  Everything else is
 * nmi_search_grid_masked's: trees, SUC / ENMI, the all-zero guard, the [Wn][S] layout, the arg-max and key rule, blocking
 * behaviour.  NMI_OPT_SPLIT* choose the kernel, never the result: mid-size grids take the covered pixel-range kernel by the
 * masked search's rules (NMI_OPT_SPLIT 0 keeps the covered grid kernel, NMI_OPT_SPLIT 1 + NMI_OPT_SPLIT_PIXELS P forces P
 * ranges wherever they fit); NMI_OPT_CONTENT_PATH does not apply.  So all-ones render masks give nmi_search_grid_masked's
 * bits, and all-ones masks on both sides nmi_search_grid's.  Masks mean "nonzero" (bytes 1 and 2 both count).
 * NULL masks, S < 1 or Wn < 1 are NMI_ERR_INVALID_ARGUMENT.
 *
 * nmi_last_cover_counts: the first n entries of len[w][s] (layout [Wn][S]) of the latest covered search.  Blocking.
 *
 * nmi_render_points_masked / nmi_render_mesh_masked: nmi_render_points / nmi_render_mesh (d_render_stack byte-identical)
 * plus d_render_masks uint8 [S][H][W], render layout: 1 where a fragment won the pixel, 0 where it kept the clear colour --
 * exactly where the same call renders 0 with every red 0 (points) or an all-black texture (mesh), and 255 otherwise -- apart
 * from points at the far plane with colour 255, whose key is the background's (nmi_render_points).
 * Enqueued on the context's stream; a NULL d_render_masks is NMI_ERR_INVALID_ARGUMENT.
 *
 * Captured levels: nmi_level_set_coverage.  Streams: nmi_stream_submit_covered.  Not covered (yet): shard / block / RCCL forms
 * of the standalone search, the CUDAF shim.
 *
 * nmi_pack_mask_bits: bit-packed masks, the form in which a covered stream ticket carries its render masks over PCIe (1/8 of
 * the render stack's bytes).  Image i of n occupies ceil(H*W/8) bytes; pixel p (row-major, in the image's own layout) is bit
 * p % 8 (LSB first) of byte p / 8; bits past H*W in the last byte are 0 when packed here and ignored when read
 * == np.packbits(masks.reshape(n, -1) != 0, axis=1, bitorder="little").  Enqueued on the context's stream.  For a producer
 * that renders coverage on a GPU (nmi_render_*_masked), packs it there and copies only the bits to host memory.
 */
int nmi_search_grid_covered(nmi_ctx *ctx, const uint8_t *render_stack, const uint8_t *render_masks, int32_t S,
                            const uint8_t *warp_stack, const uint8_t *warp_masks, int32_t Wn, float *ratings /* nullable */,
                            int64_t *best_linear_idx, float *best_score);
int nmi_last_cover_counts(nmi_ctx *ctx, int32_t *h_counts, int32_t n);
int nmi_pack_mask_bits(nmi_ctx *ctx, const uint8_t *d_masks /*[n][H][W]*/, int32_t n, uint8_t *d_bits /*[n][ceil(H*W/8)]*/);

/*
 * Lens distortion (new): the camera frame resampled onto the pinhole camera K the renders and the warps use.  The reference's
 * tracker reads the radial-tangential coefficients Camera.k1 k2 p1 p2 [k3] into mDistCoef (src/Tracking.cc:133-144) but its
 * NMI path scores the raw mImGray (src/Tracking.cc:1871); on a rectified camera (every Camera.k* of the reference's settings
 * files is 0) the two agree.  nmi_undistort_frame maps the raw frame d_raw [H][W] (and optionally its mask d_raw_mask,
 * nonzero = usable) to the undistorted frame d_frame [H][W] and its validity mask d_frame_mask; the new camera matrix is K,
 * as in cv::undistort's default.  One resampling per frame; the warp paths then run unchanged on the result.
 *   Host: fx, fy, cx, cy = fl32(K[0], K[4], K[2], K[5]); ifx = fl32(1.0 / K[0]), ify = fl32(1.0 / K[4]) in double; the
 *   five coefficients as given (fp32).  Per output pixel (u, v), fp32 in this order:
 *     x = (u - cx) * ifx;  y = (v - cy) * ify;  x2 = x*x;  y2 = y*y;  xy = x*y;  r2 = x2 + y2
 *     rad = r2 * (k1 + r2 * (k2 + r2 * k3))
 *     dx = ((x*rad) + ((2*p1)*xy)) + (p2*(r2 + 2*x2));  dy = ((y*rad) + (p1*(r2 + 2*y2))) + ((2*p2)*xy)
 *     xs = u + fx*dx;  ys = v + fy*dy
 *   (u_d = fx x_d + cx written as a displacement: all-zero coefficients give xs = u, ys = v exactly, i.e. a byte copy and an
 *   all-ones mask).  The value at (xs, ys) is the warp stack's (reach test -2 < xs < W+1, -2 < ys < H+1, bilinear taps with
 *   a border of 0, round to nearest even, clamp to [0, 255]); the mask byte is 1 exactly where nmi_warp_stack_masked's rule
 *   holds at (xs, ys) -- the reach test, every tap with nonzero weight inside the frame and, given d_raw_mask, nonzero in
 *   it -- else 0.  Where the polynomial folds over (strong coefficients far from the centre) the result is whatever the
 *   formula gives.  Parity with cv::undistort unpinned (OpenCV is not part of the reference tree, as for the warp).
 * Enqueued on the context's stream.  NMI_ERR_INVALID_ARGUMENT, before anything is enqueued: a NULL ctx, K, dist, d_raw or
 * d_frame; K not [fx 0 cx; 0 fy cy; 0 0 1] with finite fx, fy > 0 and finite cx, cy; a non-finite coefficient;
 * d_raw == d_frame, or an output mask that aliases an input or the frame.  d_raw_mask and d_frame_mask may be NULL (no mask
 * written).
 * Captured levels: nmi_level_set_distortion.  Streams: nmi_stream_set_distortion.  Settings: nmi_config_parse_distortion
 * (include/nmi_host.h).
 */
int nmi_undistort_frame(nmi_ctx *ctx, const double K[9], const float dist[5] /* k1 k2 p1 p2 k3 */, const uint8_t *d_raw,
                        const uint8_t *d_raw_mask /* nullable */, uint8_t *d_frame, uint8_t *d_frame_mask /* nullable: no mask written */);
/*
 * Fisheye lenses (new): the four-coefficient equidistant model -- Kannala-Brandt, cv::fisheye, Kalibr "equidistant", ORB-SLAM3
 * Camera.type "KannalaBrandt8" -- of most wide-angle cameras.  nmi_undistort_frame_fisheye is nmi_undistort_frame for it, with
 * two camera matrices: K is the pinhole camera of the renders and the warps (the output), K_raw the matrix the coefficients
 * were calibrated with (the raw frame); K_raw = NULL means K.  A fisheye frame is normally undistorted onto a pinhole with a
 * shorter focal length than K_raw's, to keep its field of view.
 *   Host: cxn, cyn = fl32(K[2], K[5]); ifx = fl32(1.0 / K[0]), ify = fl32(1.0 / K[4]) in double; fx, fy, cx, cy =
 *   fl32(K_raw[0], K_raw[4], K_raw[2], K_raw[5]); k1 .. k4 as given (fp32).  Per output pixel (u, v), fp32 in this order:
 *     x = (u - cxn) * ifx;  y = (v - cyn) * ify;  r2 = x*x + y*y;  r = sqrtf(r2)
 *     theta = atan32(r):
 *         big = r > 2.414213562373095f;  mid = !big && r > 0.4142135623730950f
 *         a    = big ? -1.0f / r : mid ? (r - 1.0f) / (r + 1.0f) : r
 *         base = big ? fl32(pi/2) : mid ? fl32(pi/4) : 0.0f
 *         z = a*a
 *         q = ((8.05374449538e-2f*z - 1.38776856032e-1f)*z + 1.99777106478e-1f)*z - 3.33329491539e-1f
 *         theta = base + ((q*z)*a + a)
 *     t2 = theta*theta
 *     td = theta + theta * (t2 * (k1 + t2 * (k2 + t2 * (k3 + t2 * k4))))
 *     s  = r > 1e-8f ? td / r : 1.0f
 *     xs = cx + fx * (x * s);  ys = cy + fy * (y * s)
 *   (the arctangent written out in + - * /, a correctly rounded sqrtf and selects, not atanf, whose device and host forms
 *   differ in the last bit).  Value and mask at (xs, ys) are nmi_undistort_frame's.  There is no identity case: zero
 *   coefficients are an ideal equidistant lens, still a remap.  Where the polynomial folds over the result is whatever the
 *   formula gives.  Rays at or beyond 90 degrees from the axis are not covered (a pinhole output cannot show them).  Parity
 *   with cv::fisheye unpinned (OpenCV is not part of the reference tree).
 * Enqueued on the context's stream.  NMI_ERR_INVALID_ARGUMENT, before anything is enqueued, as for nmi_undistort_frame, with
 * K_raw (when given) held to K's rules and four coefficients.
 * Captured levels: nmi_level_set_distortion_fisheye.  Streams: nmi_stream_set_distortion_fisheye.  Settings:
 * nmi_config_parse_lens (include/nmi_host.h).
 */
int nmi_undistort_frame_fisheye(nmi_ctx *ctx, const double K[9], const double K_raw[9] /* NULL = K */, const float dist[4] /* k1 k2 k3 k4 */,
                                const uint8_t *d_raw, const uint8_t *d_raw_mask /* nullable */, uint8_t *d_frame,
                                uint8_t *d_frame_mask /* nullable: no mask written */);

/*
 * Colour and pitched camera frames (new).  The reference's tracker turns each camera frame into the grey mImGray its NMI path
 * scores with cv::cvtColor, RGB or BGR by Camera.RGB, 3 or 4 channels (src/Tracking.cc:179-183, 316-341).  A frame in one of
 * these formats is H rows of pitch bytes, row y at src + y * pitch; pitch = 0 means dense, W * bytes per pixel:
 *   NMI_FRAME_GRAY  1 byte per pixel (with a pitch: the rows are copied)
 *   NMI_FRAME_BGR, NMI_FRAME_RGB    3 bytes per pixel in that order
 *   NMI_FRAME_BGRA, NMI_FRAME_RGBA  4 bytes per pixel, the alpha byte ignored
 * Camera.RGB = 0 is BGR(A), 1 is RGB(A), as Tracking.cc chooses (nmi_config_parse_color_order, include/nmi_host.h).  The grey
 * value is OpenCV's 8-bit fixed-point rule for COLOR_{RGB,BGR,RGBA,BGRA}2GRAY, in integers:
 *   gray = (4899 R + 9617 G + 1868 B + 8192) >> 14
 * The coefficients sum to 2^14, so R = G = B = g gives g exactly.  Parity with any particular OpenCV build is unpinned (OpenCV is
 * not part of the reference tree, as for the warp and the undistortion).
 * nmi_gray_frame writes the dense grey frame d_gray [H][W] of d_src; H and W are the context's.  Enqueued on the context's
 * stream.  NMI_ERR_INVALID_ARGUMENT, before anything is enqueued: a NULL pointer, an unknown format, pitch < 0 or
 * 0 < pitch < W * bytes per pixel, d_gray overlapping the source's bytes (rows 0 .. H-1 of W * bytes per pixel each, and the
 * bytes between them).
 * Captured levels: nmi_level_set_frame_format.  Streams: nmi_stream_set_frame_format.
 *
 * Raw sensor formats (new): the same entry points, here and wherever an NMI_FRAME_* format is taken (nmi_reduce_frame, the
 * levels' and streams' setters), read what camera drivers deliver.  Every other id, 5 .. 15 included, stays unknown.
 *   NMI_FRAME_YUYV, NMI_FRAME_UYVY  packed YUV 4:2:2 (UVC / V4L2), 2 bytes per pixel, any width, dense pitch 2 W.  The grey
 *     value is the luma byte, unchanged (byte 2x of a YUYV row, 2x + 1 of a UYVY one), as COLOR_YUV2GRAY_YUY2 / _UYVY: no range
 *     expansion, and the chroma bytes are never read.
 *   NMI_FRAME_BAYER_RGGB / _GRBG / _GBRG / _BGGR  an 8-bit Bayer mosaic, 1 byte per pixel; the name is the 2x2 tile at (0, 0),
 *     row 0 then row 1.  W >= 2 and H >= 2 (of the source, for a reduced frame), else NMI_ERR_INVALID_ARGUMENT.  The rule is a
 *     bilinear demosaic followed by the weights above, in integers, with one rounding.  With p(dx, dy) the mosaic byte at
 *     (x + dx, y + dy), and R4, G4, B4 four times the channels:
 *       red site     R4 = 4 p(0,0)   G4 = p(-1,0) + p(1,0) + p(0,-1) + p(0,1)   B4 = p(-1,-1) + p(1,-1) + p(-1,1) + p(1,1)
 *       blue site    as the red site, with R4 and B4 exchanged
 *       green site in a red row    R4 = 2 (p(-1,0) + p(1,0))   G4 = 4 p(0,0)   B4 = 2 (p(0,-1) + p(0,1))
 *       green site in a blue row   as in a red row, with R4 and B4 exchanged
 *       gray = (4899 R4 + 9617 G4 + 1868 B4 + 32768) >> 16
 *     A flat mosaic of value g gives g exactly, and the value is within 0.5 of the exact (4899 R4 + 9617 G4 + 1868 B4) / 65536.
 *     Coordinates outside the frame are reflected without repeating the edge (-1 -> 1, W -> W - 2, and the same in y), which
 *     keeps the colour phase of the mosaic.  The frame is the W x H (for nmi_reduce_frame the f W x f H) pixels the call covers:
 *     a pitch's padding and spare columns or rows are never read, and the last covered column and row reflect inwards.  A caller
 *     who crops by offsetting d_src by an odd number of columns or rows changes the pattern and must pass the one that results:
 *     RGGB one column in is GRBG, one row down GBRG, both BGGR.  Parity with OpenCV's demosaicing is unpinned.
 *   NV12 / NV21 / I420 (hardware video decoders) need no id: their luma plane is H rows of pitch bytes, which is NMI_FRAME_GRAY
 *     with that pitch.  A stream then copies only the H luma rows of the host buffer, never the chroma plane behind them.
 * Not covered: packed 10 / 12-bit mosaics (16-bit mosaics are NMI_FRAME_BAYER16_*, deep grey frames NMI_FRAME_GRAY16 and its
 * packed forms, all below), edge-aware demosaicing, chroma of any kind, planar 4:2:2 / 4:4:4.
 */
#define NMI_FRAME_GRAY 0
#define NMI_FRAME_BGR 1
#define NMI_FRAME_RGB 2
#define NMI_FRAME_BGRA 3
#define NMI_FRAME_RGBA 4
#define NMI_FRAME_YUYV 16        /* Y0 U Y1 V ...   2 bytes per pixel, luma at byte 2x     */
#define NMI_FRAME_UYVY 17        /* U Y0 V Y1 ...   2 bytes per pixel, luma at byte 2x + 1 */
#define NMI_FRAME_BAYER_RGGB 32  /* 1 byte per pixel; the name is the 2x2 tile at (0,0): row 0 then row 1 */
#define NMI_FRAME_BAYER_GRBG 33
#define NMI_FRAME_BAYER_GBRG 34
#define NMI_FRAME_BAYER_BGGR 35
#define NMI_FRAME_GRAY16 48      /* 2 bytes per pixel, little-endian unsigned, H rows of pitch bytes; dense pitch 2 W */
/* Deep raw formats ("Deep frames" below: each unpacks to the GRAY16 container; 51 stays unknown) */
#define NMI_FRAME_GRAY16_BE 50   /* 2 bytes per pixel, big-endian unsigned */
#define NMI_FRAME_MONO10P 52     /* PFNC Mono10p: 4 pixels in 5 bytes, lsb-packed */
#define NMI_FRAME_MONO12P 53     /* PFNC Mono12p: 2 pixels in 3 bytes, lsb-packed */
#define NMI_FRAME_RAW10 54       /* CSI-2 RAW10 / V4L2 Y10P: 4 pixels in 5 bytes, the low bits in the fifth */
#define NMI_FRAME_RAW12 55       /* CSI-2 RAW12 / V4L2 Y12P: 2 pixels in 3 bytes, the low bits in the third */
#define NMI_FRAME_BAYER16_RGGB 56 /* 2 bytes per site, little-endian; named as the 8-bit mosaics */
#define NMI_FRAME_BAYER16_GRBG 57
#define NMI_FRAME_BAYER16_GBRG 58
#define NMI_FRAME_BAYER16_BGGR 59
int nmi_gray_frame(nmi_ctx *ctx, const uint8_t *d_src, int32_t format, int64_t pitch /* bytes, 0 = dense */, uint8_t *d_gray /* [H][W] */);

/*
 * Full-size camera frames (new).  The reference searches at a fraction of the camera's size: "ZU-MAV 1920x1080 frame
 * downsampled to 960x540" (BASELINE.json configs[2]; Examples/Monocular/ETH_small.yaml:23-24).  nmi_reduce_frame makes the grey
 * frame d_gray [H][W] of the search size -- H and W are the context's -- from a source of f * H rows of f * W pixels in an
 * NMI_FRAME_* format, f = factor = 1 .. 4.  Row y is at d_src + y * pitch; pitch = 0 means dense, f * W * bytes per pixel.  A
 * source with spare columns or rows is cropped by passing its real pitch: 1241x376 at f = 2 gives 620x188.
 * Each source pixel is first turned grey by nmi_gray_frame's rule (GRAY: the byte itself); output pixel (x, y) is then the box
 * average of the f x f grey values at (f x .., f y ..), rounded from their integer sum s:
 *   f = 1   s (the call is nmi_gray_frame)
 *   f = 2   (s + 2) >> 2
 *   f = 3   (s + 4) / 9
 *   f = 4   q + (r > 8 || (r == 8 && (q & 1))),  q = s >> 4, r = s & 15    (round half to even)
 * each within 0.5 of the exact mean.  They are the integer forms of what cv::resize(INTER_AREA) is understood to compute at
 * integer scales: its 2x2 fast path for f = 2 (halves round up), rint(fl32(s) * fl32(1 / f^2)) for f = 3 and 4, which they
 * equal for every possible s.  Parity with any particular OpenCV build is unpinned, as for the warp, the undistortion and the
 * colour rule.
 * Mask: d_mask[y][x] = 1 where all f x f bytes of d_src_mask (dense uint8 [f*H][f*W]) are nonzero, else 0; written only when
 * both mask pointers are given.
 * Enqueued on the context's stream.  NMI_ERR_INVALID_ARGUMENT, before anything is enqueued and with the outputs untouched: a NULL
 * ctx, d_src or d_gray, an unknown format, a factor outside 1 .. 4, pitch < 0 or 0 < pitch < f * W * bytes per pixel, exactly
 * one of the two mask pointers given, an output overlapping the source's bytes (rows 0 .. f*H-1 and the bytes between them),
 * the source mask or the other output.
 * Captured levels: nmi_level_set_frame_reduction.  Streams: nmi_stream_set_frame_reduction.  The search-size camera model of a
 * full-size settings file: nmi_config_reduce (include/nmi_host.h).
 * Not covered: non-integer scales, factors above 4, a fused reduce + undistort node, resolution pyramids inside
 * nmi_relocalize_with_strategy.
 */
int nmi_reduce_frame(nmi_ctx *ctx, const uint8_t *d_src, int32_t format, int64_t pitch /* bytes, 0 = dense */,
                     int32_t factor /* 1..4 */, const uint8_t *d_src_mask /* nullable, dense [f*H][f*W] */,
                     uint8_t *d_gray /* [H][W] */, uint8_t *d_mask /* nullable, [H][W] */);

/*
 * Deep frames (new).  Thermal, SWIR, NIR, depth and machine-vision cameras deliver more than 8 bits per pixel (GenICam Mono10 /
 * Mono12 / Mono16, V4L2 Y10 / Y12 / Y16): NMI_FRAME_GRAY16 is their unpacked container, 2 bytes per pixel, little-endian
 * unsigned, taken wherever an NMI_FRAME_* value is (nmi_gray_frame, nmi_reduce_frame, the levels' and streams' frame setters).
 * Ids 47 and 49 stay unknown.  d_src and a non-zero pitch must be multiples of 2 (NMI_ERR_INVALID_ARGUMENT), the pitch and
 * overlap rules are the other formats' with 2 bytes per pixel, and a frame has at most 2^32 - 1 pixels.
 * The search bins 256 levels, so a deep pixel becomes 8-bit by a tone map, nmi_tone_map: per context (nmi_set_tone_map; read
 * by nmi_gray_frame, nmi_reduce_frame, nmi_tone_lut and nmi_tone_tile_luts at call time), per level and per stream.  It is ignored for every other
 * format.  The rule is integers throughout.  M = 2^bits - 1; v = min(raw, M) (values above the declared depth saturate); N =
 * the pixels the call covers, W x H of the source or f W x f H for a reduced frame (a pitch's padding and spare rows or columns
 * are never read); h[v] = the exact count of v over them, c[v] its inclusive running sum.  A frame mask does not change h; a
 * valid range (below) does: h and N are then those of the valid pixels.
 *   NMI_TONE_SHIFT       out = v >> (bits - 8)
 *   NMI_TONE_WINDOW      v <= lo: 0; otherwise v >= hi: 255; otherwise ((v - lo) * 255 + ((hi - lo) >> 1)) / (hi - lo)
 *   NMI_TONE_PERCENTILE  k_lo = N * p_lo / 10000, k_hi = N * p_hi / 10000 (64-bit, floor); lo = the smallest v with c[v] > k_lo,
 *                        hi = the smallest v with c[v] >= N - k_hi; then WINDOW(lo, hi), whose order of cases makes a flat frame
 *                        (hi == lo) all 0.  p_lo = p_hi = 0 is the min-max stretch.
 *   NMI_TONE_EQUALIZE    h'[v] = plateau ? min(h[v], plateau) : h[v], c' its inclusive running sum, T = c'[M], vmin = the smallest
 *                        v with h[v] > 0, c0 = h'[vmin].  T == c0: every pixel 0.  Otherwise, for v >= vmin,
 *                        out = ((c'[v] - c0) * 255 + ((T - c0) >> 1)) / (T - c0) with 64-bit products, and 0 below vmin.  This is
 *                        cv::equalizeHist's rule carried to 16 bits; with a plateau, the thermal cameras' plateau equalisation.
 *                        Parity with an OpenCV build is unpinned.
 *   NMI_TONE_TABLE       out = d_lut[v]: for callers who hold one mapping over a sequence (nmi_tone_lut makes one from a frame).
 *   NMI_TONE_CLAHE       (mode 6; 5 stays unknown) contrast-limited equalisation per tile, the standard answer where one hot
 *                        object or a cold sky would take most of a global table's levels.  The source (Ws x Hs = f W x f H) is
 *                        cut into tiles_x x tiles_y tiles: column x is in tile column ((2 x + 1) tiles_x) / (2 Ws), row y in tile
 *                        row ((2 y + 1) tiles_y) / (2 Hs); no tile is empty, and tiles differ in size where the size does not
 *                        divide.  Per tile t of n_t pixels with exact counts h_t and L = M + 1 levels: plateau P == 0: c'' = the
 *                        running sum of h_t.  P >= 1: E = sum max(h_t[v] - P, 0), c' = the running sum of min(h_t[v], P), q = E / L,
 *                        r = E % L, step = max(L / r, 1), c''[v] = c'[v] + q (v + 1) + (r ? min(r, v / step + 1) : 0): every level
 *                        gets q of the excess and levels 0, step, 2 step, ... one more until r are given out (cv::CLAHE's
 *                        redistribution in closed form); c''[M] == n_t.  T_t[v] = (c''[v] 255 + (n_t >> 1)) / n_t, 64-bit products.
 *                        Per pixel: ax = (2 x + 1) tiles_x - Ws, dx = 2 Ws, i0 = floor(ax / dx) (-1 in the first half tile),
 *                        wx = ((ax - i0 dx) 256) / dx, i1 = i0 + 1, both clamped to 0 .. tiles_x - 1; j0, j1, wy likewise from y;
 *                        out = ((T[j0][i0][v] (256 - wx) + T[j0][i1][v] wx) (256 - wy)
 *                             + (T[j1][i0][v] (256 - wx) + T[j1][i1][v] wx) wy + 32768) >> 16.
 *                        Parity with an OpenCV build is unpinned (it pads by reflection and interpolates in float).
 * A reduced frame maps each source pixel, then takes nmi_reduce_frame's rounded box average of the 8-bit values; the statistics
 * (CLAHE: the tiles and the blend too) are the full-size frame's.  SHIFT, WINDOW and TABLE cost the conversion kernel alone;
 * PERCENTILE and EQUALIZE put a histogram kernel and two small table kernels in front of it, CLAHE a tile-histogram kernel and a
 * tile-table kernel in front of a conversion kernel of its own (four table reads per source pixel), on the same stream (in a
 * level: in the captured graph, from d_frame at every replay; in a stream: for every submitted frame).  With a lens distortion
 * the grey frame is made first and undistorted second (two nodes, as for a mosaic).
 * A CLAHE setting adds device memory to whoever converts with it -- the context (at the first nmi_gray_frame, nmi_reduce_frame
 * or nmi_tone_tile_luts), a level, a stream, each for itself: tiles_x tiles_y (4 * 2^bits + 65536) bytes + 256, that is 20 MiB at
 * 8 x 8 tiles of 16 bits, 8 MiB at 14 bits; kept until the owner is destroyed (a level drops it when its format leaves GRAY16).
 * nmi_tone_map_default fills *tm with SHIFT, bits 16 (the setting of a new context, level or stream; also what a NULL tm
 * sets).  NMI_ERR_INVALID_ARGUMENT, the setting left as it was: bits outside 8 .. 16, an unknown mode, a non-zero reserved
 * word (tiles_x and tiles_y count as such under every mode but CLAHE), WINDOW without 0 <= lo < hi <= M, PERCENTILE with a
 * negative share or p_lo + p_hi >= 10000, EQUALIZE or CLAHE with a negative plateau, TABLE with a NULL d_lut, CLAHE with a tile
 * count outside 1 .. 8 or tiles_x > W or tiles_y > H of the context.  Only the fields of the chosen mode (and bits, tiles_x,
 * tiles_y, reserved) are read.
 * nmi_level_set_tone_map captures the level again (waiting for a replay in flight), like the other level setters;
 * nmi_stream_set_tone_map holds for later submissions.
 * nmi_tone_lut writes the table the context's tone map gives for the frame at d_src (f H rows of pitch bytes, f W GRAY16 pixels
 * each, f = factor) into d_lut, all 65,536 entries: entry i is the 8-bit value of v = min(i, M).  Enqueued on the context's
 * stream; with h_window it blocks and returns {lo, hi}: PERCENTILE the chosen pair, EQUALIZE the smallest and largest value
 * present, WINDOW the given pair, SHIFT and TABLE {0, M}.  NMI_ERR_INVALID_ARGUMENT before anything is enqueued: a NULL ctx,
 * d_src or d_lut, a factor outside 1 .. 4, an odd d_src or pitch, 0 < pitch < 2 f W, d_lut overlapping the source's bytes.
 * Under CLAHE there is no single table: NMI_ERR_UNSUPPORTED, nothing enqueued, d_lut untouched.
 * nmi_tone_tile_luts is its CLAHE counterpart: T_t of every tile into d_luts [tiles_y][tiles_x][65536] (entry i the value of
 * min(i, M)), enqueued on the context's stream; with h_counts it blocks and returns the tiles' pixel counts n_t.  The argument
 * checks are nmi_tone_lut's (d_luts' tiles_x tiles_y 65,536 bytes may not meet the source's); under any other mode
 * NMI_ERR_UNSUPPORTED, nothing enqueued, d_luts untouched.
 * Valid range.  Deep sensors reserve values for "no measurement": a depth stream writes 0 where it has no return, a 12-bit
 * sensor in a 16-bit container 65535 for a dead pixel, a thermal core parks saturated pixels at its top code.  A valid range
 * keeps them out of the statistics and marks them in a mask the masked and covered searches take (nmi_warp_stack_masked's frame
 * mask).  nmi_set_valid_range (per context, read at call time by nmi_gray_frame, nmi_reduce_frame, nmi_tone_lut,
 * nmi_tone_tile_luts and nmi_deep_frame) takes 0 <= lo <= hi <= 65535, else NMI_ERR_INVALID_ARGUMENT with the setting left as it
 * was.  (0, 65535) is off: the setting of every new context, under which every output byte and every kernel launched is what it
 * was without this setting.  The range is kept, and ignored, under every format other than GRAY16, like the tone map;
 * nmi_tone_map itself is untouched.
 *   Validity    a source pixel is valid iff lo <= raw <= hi, raw being the container's value BEFORE it saturates to M: (0, 4095)
 *               at bits = 12 drops a 65535 sentinel that would otherwise count as 4095.
 *   Statistics  h[v] counts valid pixels only, and N is their number, in PERCENTILE's k_lo, k_hi and c[v] >= N - k_hi and in
 *               EQUALIZE's T; CLAHE's h_t and n_t are per tile, over its valid pixels.  nmi_tone_lut's h_window and
 *               nmi_tone_tile_luts' h_counts report the valid pixels' values and numbers.
 *   No pixels   a global mode with N == 0: the table is all 0 and the window {0, 0}.  A CLAHE tile with n_t == 0: T_t is SHIFT's
 *               table, min(i, M) >> (bits - 8) -- a neutral table, so that the valid pixels of neighbouring tiles that blend
 *               with it are not pulled to black.
 *   Grey bytes  an invalid pixel still becomes table[min(raw, M)] (under CLAHE: the blend), as before: only the tables change,
 *               and SHIFT, WINDOW and TABLE give the same grey bytes with and without a range.
 *   Mask        the validity mask is dense uint8 [H][W] at the search size, 1 or 0: 1 iff all f x f source pixels under (x, y)
 *               are valid (nmi_reduce_frame's "all of them" rule) and, where a frame mask is given, its byte at (x, y) is
 *               nonzero.
 * nmi_reduce_frame's own mask pair keeps its rule and its argument checks; when both mask pointers are given, the source is
 * GRAY16 and a range is on, d_mask is additionally ANDed with validity.
 * nmi_deep_frame is the entry for a frame mask at the search size, which nmi_gray_frame cannot take: the GRAY16 source at d_src
 * (f H rows of pitch bytes, f = factor) under the context's tone map and range -> d_gray, the grey frame nmi_gray_frame /
 * nmi_reduce_frame give, and d_mask, the validity mask ANDed with d_frame_mask (nullable), both written by one conversion kernel
 * (range off: every pixel is valid).  Enqueued on the context's stream.  NMI_ERR_INVALID_ARGUMENT, before anything is enqueued
 * and with the outputs untouched: a NULL ctx, d_src, d_gray or d_mask, a factor outside 1 .. 4, an odd d_src or pitch, pitch < 0
 * or 0 < pitch < 2 f W, any two of the source's bytes, the frame mask and the two outputs overlapping.
 * The masked chain on a deep frame is then nmi_deep_frame, nmi_undistort_frame* with d_mask as its raw mask (if distorted),
 * nmi_warp_stack_masked with the result as its frame mask, nmi_search_grid_masked or nmi_search_grid_covered.
 * Captured levels and streams have a range of their own, like their tone map: nmi_level_set_valid_range and
 * nmi_stream_set_valid_range (below, beside the other setters).  The context's nmi_set_valid_range governs the standalone entries
 * only and never reaches a level or a stream.
 * Deep raw formats (new).  What deep sensors put on the wire is rarely the container: GigE / USB3 Vision cameras pack Mono10p /
 * Mono12p, CSI-2 sensors MIPI RAW10 / RAW12 (V4L2 Y10P / Y12P), colour machine-vision cameras send a Bayer mosaic in 16-bit
 * words, PGM files and some thermal cores are big-endian.  Nine formats, taken wherever NMI_FRAME_GRAY16 is (nmi_gray_frame,
 * nmi_reduce_frame, the levels' and streams' frame setters), each UNPACK to a container pixel u(x, y), right-justified, whose
 * depth the tone map's bits states.  With b the bytes of a row (row y starts at d_src + y * pitch):
 *   NMI_FRAME_GRAY16_BE   2 bytes per pixel: u(x) = b[2x] << 8 | b[2x+1]
 *   NMI_FRAME_MONO10P     PFNC lsb-packed, 4 pixels in 5 bytes: pixel k of the row is bits [10k, 10k + 10) of the row read as one
 *                         little-endian bit string (bit j of the string is bit j % 8 of b[j / 8])
 *   NMI_FRAME_MONO12P     PFNC lsb-packed, 2 pixels in 3 bytes: pixel k is bits [12k, 12k + 12) of that string
 *   NMI_FRAME_RAW10       CSI-2 / Y10P, 4 pixels in 5 bytes: u(4g + i) = b[5g + i] << 2 | ((b[5g + 4] >> 2i) & 3), i = 0 .. 3
 *   NMI_FRAME_RAW12       CSI-2 / Y12P, 2 pixels in 3 bytes: u(2g) = b[3g] << 4 | (b[3g + 2] & 15), u(2g + 1) = b[3g + 1] << 4 |
 *                         (b[3g + 2] >> 4)
 *   NMI_FRAME_BAYER16_RGGB / _GRBG / _GBRG / _BGGR   2 bytes per site, little-endian: u = (4899 R4 + 9617 G4 + 1868 B4 + 32768)
 *                         >> 16, with R4, G4, B4 the 8-bit mosaics' bilinear sums (nmi_gray_frame) over the raw 16-bit sites, the
 *                         same reflected edges and the same pattern naming.  A site is not saturated to M first (u is, like any
 *                         container pixel, afterwards); the sum stays below 2^32, and a flat mosaic of g gives g.
 * A call on one of them is, byte for byte, the unpacking into a dense container followed by the same call on NMI_FRAME_GRAY16:
 * tone map, statistics, CLAHE tiles and blends, reduction and valid range are all taken on u (for a mosaic: on the demosaiced
 * grey value).  That is also how it runs: one unpack kernel writes the container (2 f W f H bytes of device memory, kept by
 * the context, level or stream beside its tone tables), and the GRAY16 kernels read it.  GRAY16 itself and the 8-bit formats
 * launch what they always did.
 * Rows: every row starts on a byte; pitch = 0 means dense, Ws 10 / 8, Ws 12 / 8 or 2 Ws bytes for a source row of Ws = f W
 * pixels (nmi_frame_row_bytes).  Whole groups only: Ws % 4 == 0 for the 10-bit formats, Ws % 2 == 0 for the 12-bit ones, else
 * NMI_ERR_INVALID_ARGUMENT.  A packed row and its base may sit at any byte address, and a packed pitch may be odd; the 2-byte
 * formats keep GRAY16's rules (even base, even pitch), BAYER16 the mosaics' Ws, Hs >= 2.  The pitch, overlap and frame-size
 * checks are the other formats' with the row's true byte count in place of W * bytes per pixel; nothing past a row's last byte
 * is read.  A stream copies f H rows of the packed row bytes: 1.25 or 1.5 bytes per pixel on the wire instead of 2.
 * nmi_frame_row_bytes: the dense bytes of a row of `width` pixels in any NMI_FRAME_* format; 0 for an unknown format or a width
 * that is not whole groups.  Host only, no context.
 * nmi_unpack_frame writes the container itself: f H rows of pitch bytes at d_src in `format` -> d_gray16, dense uint16 [f H][f W]
 * (H and W the context's).  Enqueued on the context's stream.  nmi_tone_lut, nmi_tone_tile_luts and nmi_deep_frame take no
 * format: a caller with a packed, mosaic or big-endian source feeds them nmi_unpack_frame's output as GRAY16 with pitch 0.
 * NMI_ERR_INVALID_ARGUMENT before anything is enqueued, d_gray16 untouched: a NULL pointer, a factor outside 1 .. 4, the pitch,
 * alignment, group and overlap rules above (d_gray16's 2 f W f H bytes may not meet the source's; d_gray16 is 2-byte aligned),
 * any format other than these nine (GRAY16 included: it is its own container).
 * Not covered: GigE Vision Mono12Packed (the GVSP layout, not Mono12p), MSB-justified containers, RAW14, packed Bayer (10 / 12-bit
 * mosaics in 5 / 3-byte groups), rows that do not start on a byte, CLAHE of
 * 8-bit formats, caller-supplied tile tables, more than 8 x 8 tiles, temporal smoothing of the window (TABLE is the hook: smooth
 * on the host, pass the table), statistics under the caller's own frame mask, validity for the 8-bit formats (saturated 0 /
 * 255), hole filling or inpainting, a way to read a level's validity mask back other than through its warp masks, a per-pixel
 * weight instead of a mask, renormalised CLAHE blends beside an empty tile, the CUDAF shim.
 */
#define NMI_TONE_SHIFT 0
#define NMI_TONE_WINDOW 1
#define NMI_TONE_PERCENTILE 2
#define NMI_TONE_EQUALIZE 3
#define NMI_TONE_TABLE 4
#define NMI_TONE_CLAHE 6 /* (not 5: mode 5 stays an unknown mode, NMI_ERR_INVALID_ARGUMENT) */

typedef struct nmi_tone_map {
    int32_t mode;         /* NMI_TONE_* */
    int32_t bits;         /* significant bits of the container, 8 .. 16 */
    int32_t lo, hi;       /* WINDOW: 0 <= lo < hi <= 2^bits - 1 */
    int32_t p_lo, p_hi;   /* PERCENTILE: shares of the pixels cut at each end, in 1/10000; >= 0, p_lo + p_hi < 10000 */
    int32_t plateau;      /* EQUALIZE, CLAHE: per-level count limit (CLAHE: per tile), 0 = none; >= 0 */
    int32_t tiles_x, tiles_y; /* CLAHE: tiles per axis, 1 .. 8, tiles_x <= W, tiles_y <= H; 0 under every other mode (they were
                                 the first two reserved words: layout and size are unchanged) */
    int32_t reserved[3];  /* must be 0 */
    const uint8_t *d_lut; /* TABLE: device uint8 [65536], must stay valid and unchanged while the setting is in force */
} nmi_tone_map;

int nmi_tone_map_default(nmi_tone_map *tm);
int nmi_set_tone_map(nmi_ctx *ctx, const nmi_tone_map *tm /* NULL = the default */);
int nmi_tone_lut(nmi_ctx *ctx, const uint8_t *d_src, int64_t pitch /* bytes, 0 = dense */, int32_t factor /* 1..4 */,
                 uint8_t *d_lut /* [65536] */, int32_t h_window[2] /* nullable */);
int nmi_tone_tile_luts(nmi_ctx *ctx, const uint8_t *d_src, int64_t pitch /* bytes, 0 = dense */, int32_t factor /* 1..4 */,
                       uint8_t *d_luts /* [tiles_y][tiles_x][65536] */, int32_t *h_counts /* nullable, [tiles_y][tiles_x] */);
int nmi_set_valid_range(nmi_ctx *ctx, int32_t lo, int32_t hi /* 0 <= lo <= hi <= 65535; (0, 65535) = off */);
int nmi_deep_frame(nmi_ctx *ctx, const uint8_t *d_src, int64_t pitch /* bytes, 0 = dense */, int32_t factor /* 1..4 */,
                   const uint8_t *d_frame_mask /* nullable, dense [H][W], search size */, uint8_t *d_gray /* [H][W] */,
                   uint8_t *d_mask /* [H][W] */);
int64_t nmi_frame_row_bytes(int32_t format, int32_t width);
int nmi_unpack_frame(nmi_ctx *ctx, const uint8_t *d_src, int32_t format, int64_t pitch /* bytes, 0 = dense */, int32_t factor /* 1..4 */,
                     uint16_t *d_gray16 /* [f*H][f*W] */);

/*
 * Render-stack producer for coloured point clouds: replaces Rendering<4>::renderToTextureOnGPU
 * (Thirdparty/Localization/rendering.hpp:530-630, nmi_prop_RENDER 4, shaders/ShadingWithColor.*) for S camera
 * translations of one pose -- no OpenGL.  nmi_render_mvp builds Projection * glm::lookAt for one view exactly as
 * rendering.hpp:196-202,547-553 (column-major float[16] like glm); nmi_render_points draws the cloud into
 * d_render_stack [S][H][W] (uint8, bottom-up rows like the GL texture, background 255).  d_xyz: float [N][3] vertices
 * (loadXYZ output, objloader.cpp:257-260), d_red: float [N] red colour component (objloader.cpp:261: file value / 256).
 * Point rule: a point is drawn iff its clip coordinate w is a positive normal float and |x|, |y|, |z| <= w (a NaN coordinate
 * is not drawn); odd sizes are centred on floor(xw) + 0.5, even sizes on floor(xw + 0.5); depth = min(round(zw * (2^24 - 1)),
 * 2^24 - 1), so a point at the far plane has the largest depth and loses to anything nearer; colour = round(clamp(red, 0, 1)
 * * 255), a NaN red giving 0.  Each pixel keeps the smallest depth << 8 | colour: among equal 24-bit depths the SMALLER red
 * wins, where GL_LESS would keep the point drawn first (a deliberate deviation: one atomicMin per point and view).  A second
 * deliberate deviation: the reference clears depth to 1.0 and tests GL_LESS (rendering.hpp:294-297), so it draws no point at
 * the far plane; here such a point is drawn at depth 2^24 - 1, behind everything nearer, and covered -- except with colour
 * 255, whose key is the background's: it leaves 255 and is not covered (nmi_render_points_masked).
 * point_size: NaN is NMI_ERR_INVALID_ARGUMENT; otherwise the size is rounded to nearest, floor(point_size + 0.5) in float,
 * and clamped to [1, 64] before any conversion to int, so 1e10 and inf draw 64 x 64 sprites.  The same rule holds for
 * nmi_level_create / nmi_level_create_block.
 * Enqueued on the context's stream.  Parity with an OpenGL driver's rasteriser is unpinned (kernel comment).
 */
typedef struct nmi_render_params {
    double fx, fy, cx, cy;  /* Camera.fx .. Camera.cy (localization.cpp:149-152) */
    float near_plane;       /* NMI.Render.NearPlane */
    float far_plane;        /* NMI.Render.FarPlane  */
    float point_size;       /* NMI.Render.PointSize -> glPointSize (rendering.hpp:307) */
} nmi_render_params;
int nmi_render_mvp(const nmi_render_params *rp, const float cam_pos[3], const float cam_look_at[3], const float cam_up[3],
                   const float translation[3], float out_mvp[16]);
int nmi_render_points(nmi_ctx *ctx, const float *d_xyz, const float *d_red, int64_t n_points, const float *h_mvps, int32_t S,
                      float point_size, uint8_t *d_render_stack);

/*
 * Render-stack producer for textured meshes (nmi_prop_RENDER 1, the reference's default): replaces
 * Rendering<1>::renderToTextureOnGPU (rendering.hpp:530-630, shaders/ShadingWithTexture.*) -- no OpenGL.
 *   nmi_texture_create  takes the RGB8 image exactly as loadBMP_custom passes it to glTexImage2D (texture.cpp:31-86: row 0
 *                       = v 0, three bytes per texel in file order; the shader weighs byte 0 with 0.299, byte 1 with 0.587,
 *                       byte 2 with 0.114), builds the mip chain glGenerateMipmap would (2x2 box, RGB8 per level) and keeps
 *                       per-level luma on the device.  Sides up to 32,768 texels and at most 2^30 texels in the whole
 *                       pyramid (a 28,000 x 28,000 image), else NMI_ERR_UNSUPPORTED.
 *   nmi_render_mesh     d_xyz float [3*T][3] and d_uv float [3*T][2]: the expanded per-corner arrays loadOBJ produces
 *                       (objloader.cpp:140-224); h_mvps as for nmi_render_points; output uint8 [S][H][W], bottom-up rows,
 *                       background 255.  Back faces culled (counter-clockwise front), depth test LESS, GL_REPEAT,
 *                       GL_LINEAR / GL_LINEAR_MIPMAP_LINEAR.  Triangles are clipped against the near plane in clip space
 *                       (a ground plane passing under the camera keeps its visible part).  Among fragments of equal 24-bit
 *                       depth the triangle drawn first (lowest index) wins, as GL_LESS leaves it.  At most 2^30 - 1 triangles.
 *                       GL_REPEAT is exact while |u w_l - 0.5| < 2^24 - w_l on every sampled level l (v, h_l likewise);
 *                       beyond that, and for non-finite uv, a sample reads some texel inside the level, not the repeated one.
 * Enqueued on the context's stream.  Parity with an OpenGL driver is unpinned (kernel comment).
 */
typedef struct nmi_texture nmi_texture;
int nmi_texture_create(nmi_ctx *ctx, const uint8_t *h_rgb, int32_t tex_width, int32_t tex_height, nmi_texture **out);
int nmi_texture_destroy(nmi_texture *tex);
int nmi_render_mesh(nmi_ctx *ctx, const float *d_xyz, const float *d_uv, int64_t n_triangles, const nmi_texture *tex,
                    const float *h_mvps, int32_t S, uint8_t *d_render_stack);
/* coverage forms (see nmi_search_grid_covered above) */
int nmi_render_points_masked(nmi_ctx *ctx, const float *d_xyz, const float *d_red, int64_t n_points, const float *h_mvps, int32_t S,
                             float point_size, uint8_t *d_render_stack, uint8_t *d_render_masks);
int nmi_render_mesh_masked(nmi_ctx *ctx, const float *d_xyz, const float *d_uv, int64_t n_triangles, const nmi_texture *tex,
                           const float *h_mvps, int32_t S, uint8_t *d_render_stack, uint8_t *d_render_masks);

/*
 * Render-stack producer for vertex-coloured meshes (new): a triangle mesh with one colour per corner and no texture -- what
 * Poisson / TSDF reconstructions and MeshLab, CloudCompare or Open3D exports ("v x y z r g b") hand out.  It stands for the draw
 * the reference's Rendering<>::renderToTextureOnGPU (rendering.hpp:175,530-630) would make of such a mesh with
 * shaders/ShadingWithColor.* -- the interpolated vertex colour passed straight through -- read back by glReadPixels(GL_RED)
 * (rendering.hpp:520); the reference itself ships that shader for points only (allProperties.hpp:40: "other rendering options can
 * be added").  No OpenGL.
 *   nmi_render_mesh_colored  d_xyz float [3*T][3] as for nmi_render_mesh; d_red float [3*T]: the red component of each corner, in
 *                            the order of d_xyz (nmi_map_load_obj_colored, include/nmi_host.h).  Everything in front of the
 *                            fragment shader is nmi_render_mesh's: culling, near-plane clipping (the colour is cut as uv is),
 *                            top-left fill rule, 24-bit depth with the triangle drawn first winning ties, background 255, at
 *                            most 2^30 - 1 triangles.  Per pixel the colour is interpolated perspective-correctly,
 *                            c = (red / w) / (1 / w) over the window as nmi_render_mesh interpolates u, and the grey level is
 *                            the point renderer's colour rule: round(clamp(c, 0, 1) * 255), a NaN giving 0.
 *   nmi_render_mesh_colored_masked   the same plus d_render_masks (see nmi_search_grid_covered above): 1 where a fragment won.
 * Enqueued on the context's stream.  NMI_ERR_INVALID_ARGUMENT as for nmi_render_mesh (a NULL d_xyz or d_red with triangles to
 * draw, S < 1, NULL outputs).  Parity with an OpenGL driver is unpinned (kernel comment, nmi_mesh.hip).
 */
int nmi_render_mesh_colored(nmi_ctx *ctx, const float *d_xyz, const float *d_red, int64_t n_triangles, const float *h_mvps, int32_t S,
                            uint8_t *d_render_stack);
int nmi_render_mesh_colored_masked(nmi_ctx *ctx, const float *d_xyz, const float *d_red, int64_t n_triangles, const float *h_mvps,
                                   int32_t S, uint8_t *d_render_stack, uint8_t *d_render_masks);

/*
 * Depth maps (new): the map's own geometry as the search image.  For a depth camera (or any map without an appearance attribute:
 * a LiDAR cloud without intensity, a CAD model, an untextured reconstruction) the render shows, per pixel, the DEPTH of whatever
 * won it instead of its colour.  Nothing in front of the shader changes -- culling, clipping, splats, bins, the 24-bit depth
 * test and its tie rules are those of nmi_render_points / nmi_render_mesh -- and the output is a pure function of the winner's
 * 24-bit window depth d.  The rule, in fp32, every operation rounded on its own, both divisions IEEE divisions:
 *     u    = (float)(2^24 - 1 - d) / (2^24 - 1)                       1 - zw; the numerator is exact
 *     den  = near + u * (far - near)
 *     z    = (near * far) / den                                       eye-space Z: what RealSense / Kinect-class cameras report
 *     v    = clamp((uint32)(z * scale + 0.5), 1, 65535)               raw 16-bit depth; 0 is kept for "nothing there"
 *     grey = v <= lo ? 0 : v >= hi ? 255 : ((v - lo) * 255 + ((hi - lo) >> 1)) / (hi - lo)      NMI_TONE_WINDOW(lo, hi)'s integer rule
 * A pixel nothing won has v = 0 and grey = 255, the background every renderer clears to.  The grey is therefore what
 * NMI_TONE_WINDOW(lo, hi) makes of v: a depth frame brought in through nmi_deep_frame (or a level's intake) with that tone map and
 * the valid range (1, 65535) and the depth render see depth through one mapping ("Depth maps").
 * near_plane and far_plane must be those of the projection inside h_mvps (nmi_render_mvp's rp); the rule does not read the matrices.
 *   nmi_render_points_depth  nmi_render_points_masked's draw.  d_red may be NULL (every point splats colour 0: the context then
 *                            keeps n_points floats of zeros in their place); with a d_red the
 *                            coverage is nmi_render_points_masked's byte for byte, the far-plane point of colour 255 (whose key is
 *                            the background's) included -- the colour only breaks ties between equal depths and never shows.
 *   nmi_render_mesh_depth    nmi_render_mesh's front passes on positions alone; the coverage is nmi_render_mesh_colored_masked's.
 *   d_render_stack  uint8 [S][H][W], bottom-up rows: grey.   d_render_masks (nullable) uint8 [S][H][W]: 1 where something won.
 *   d_depth16 (nullable)  uint16 [S][H][W], bottom-up rows: v -- each view's synthetic depth-camera frame; flip the rows for a
 *                         camera's top-down order.
 *   nmi_depth_shade_apply    the rule on n depths (bits above the 24th ignored): d_v and d_grey receive v and grey, either may be NULL.
 * NMI_ERR_INVALID_ARGUMENT, nothing enqueued, the context as usable as before: a NULL shade; a non-finite near_plane, far_plane or
 * scale; near_plane <= 0; far_plane <= near_plane; scale <= 0; a window outside 0 <= lo < hi <= 65535; a non-zero reserved word;
 * the renderers' own cases (a NULL context, h_mvps or d_render_stack, S < 1, a negative count, a NULL d_xyz with something to
 * draw); for nmi_depth_shade_apply n < 0, or n > 0 with a NULL d_depth24.  Enqueued on the context's stream.
 */
typedef struct nmi_depth_shade {
    float near_plane, far_plane; /* those of the projection inside h_mvps */
    float scale;                 /* raw units per world unit: 1000 = millimetres of a map in metres */
    int32_t lo, hi;              /* window in raw units, 0 <= lo < hi <= 65535 */
    int32_t reserved[3];         /* must be 0 */
} nmi_depth_shade;
int nmi_render_points_depth(nmi_ctx *ctx, const float *d_xyz, const float *d_red /* nullable */, int64_t n_points, const float *h_mvps,
                            int32_t S, float point_size, const nmi_depth_shade *shade, uint8_t *d_render_stack,
                            uint8_t *d_render_masks /* nullable */, uint16_t *d_depth16 /* nullable */);
int nmi_render_mesh_depth(nmi_ctx *ctx, const float *d_xyz, int64_t n_triangles, const float *h_mvps, int32_t S,
                          const nmi_depth_shade *shade, uint8_t *d_render_stack, uint8_t *d_render_masks /* nullable */,
                          uint16_t *d_depth16 /* nullable */);
int nmi_depth_shade_apply(nmi_ctx *ctx, const nmi_depth_shade *shade, const uint32_t *d_depth24, int64_t n, uint16_t *d_v /* nullable */,
                          uint8_t *d_grey /* nullable */);

/*
 * Map order.  What the renderers draw does not depend on the order of the points / triangles (the depth test is a
 * minimum); how fast they draw does: neighbours in memory are culled together and their fragments share cache lines of the
 * depth buffer (3 M points into 27 views: 96 us in scan order, 406 us shuffled, 116 us after nmi_sort_points).  These three
 * calls copy a map into Morton order of its positions (triangles: centroids), on the device; a loader calls them once
 * after loadXYZ / loadOBJ (objloader.cpp:140-264), whose arrays are in file order.
 * Blocking (temporary device storage: 16 bytes per record).  n below 2^32.
 *
 * The order is fully determined -- key, then input index -- by this rule, all of it in fp32, every operation rounded on its own
 * (tests/helpers/morton_np.py restates it in numpy, tests/test_map_order.py holds the device to it record for record):
 *   Position  the point itself; for a triangle the centroid ((p0 + p1) + p2) / 3, per coordinate.
 *   Placed    a position is placed iff all three coordinates have |c| <= 3.0e38f.  That is stricter than "finite": a coordinate
 *             in (3.0e38, FLT_MAX] is not placed, and neither is a triangle whose corners are finite but whose sum overflows.
 *             A NaN or an infinity anywhere in a position leaves it unplaced.  Records that are not placed come last, in input
 *             order (key 0x40000000, above every placed key).
 *   Box       per axis lo = the least and hi = the greatest coordinate of the placed positions (-0.0 below +0.0).
 *   Cell      per axis (uint32)(min(max((c - lo) / (hi - lo), 0), 1) * 1023.0f): 0 .. 1023, truncated.  Where hi - lo is 0
 *             (planar and collinear maps, identical points, lo = -0.0 with hi = +0.0) the cell is 0.  Where hi - lo overflows
 *             fp32 (say lo = -3e38, hi = 3e38) the quotient is x / inf = 0 or inf / inf = NaN, the max() turns the NaN into 0,
 *             and the cell is 0 for every record: a map that wide on all three axes comes out in input order.
 *   Key       bit 3 b + k of the key is bit b of axis k's cell (x: k = 0, y: 1, z: 2): 30 bits, x lowest.
 *   Ties      records with equal keys keep input order (the radix sort is stable and carries the input index).
 * Every record travels whole: a triangle's 9 coordinates with its 6 texture coordinates or 3 colours.
 *
 * NMI_ERR_INVALID_ARGUMENT, before anything is launched or written: a NULL context; n < 0 or n >= 2^32; with n > 0 a NULL
 * array, or an output whose bytes (n records of it) intersect those of either input or of the other output -- the gather
 * reads records while other lanes write theirs, so no overlap at any offset is allowed.  n = 0 is NMI_OK and touches nothing.
 */
int nmi_sort_points(nmi_ctx *ctx, const float *d_xyz /*[N][3]*/, const float *d_red /*[N]*/, int64_t n_points, float *d_xyz_out,
                    float *d_red_out);
int nmi_sort_triangles(nmi_ctx *ctx, const float *d_xyz /*[3*T][3]*/, const float *d_uv /*[3*T][2]*/, int64_t n_triangles,
                       float *d_xyz_out, float *d_uv_out);
/* nmi_sort_triangles for a vertex-coloured mesh: the three colours of a triangle travel with its corners. */
int nmi_sort_triangles_colored(nmi_ctx *ctx, const float *d_xyz /*[3*T][3]*/, const float *d_red /*[3*T]*/, int64_t n_triangles,
                               float *d_xyz_out, float *d_red_out);

/*
 * One whole search level on the device as a captured HIP graph: S renders of the cloud (nmi_render_points), Wn warps of the
 * frame (nmi_warp_stack) and the S x Wn search (nmi_search_grid) replay with a single hipGraphLaunch -- one chain of four
 * kernel nodes (parameter fetch + a cull of the cloud's 64-point boxes against the planes around all views; warp stack + splat of
 * the surviving points in one launch; resolve; search), no copy nodes, no branches.
 * Create once per (cloud, frame, S, Wn); nmi_level_run takes this level's S view matrices (nmi_render_mvp, float[S][16]) and
 * Wn forward homographies (nmi_warp_homographies, double[Wn][9]) and blocks until the search has posted its winner to pinned
 * host memory (the context's stream drains a few microseconds later; work enqueued on it afterwards is ordered as usual).
 * Same results as the three calls made one after the other.  The MAP is taken as it is at creation: a point-cloud level
 * keeps its own packed copy (16 bytes per point + one bounding box per 64 points), and d_xyz / d_red need not outlive the
 * call; a mesh level reads d_xyz / d_uv and the texture in place (they must stay valid and unchanged).  d_frame must stay
 * valid in place; its CONTENTS may change between runs (the next camera frame).
 */
typedef struct nmi_level nmi_level;
int nmi_level_create(nmi_ctx *ctx, const float *d_xyz, const float *d_red, int64_t n_points, const uint8_t *d_frame, int32_t S,
                     int32_t Wn, float point_size, nmi_level **out);
/* The same with the textured mesh as the map (nmi_prop_RENDER 1): d_xyz / d_uv / tex as for nmi_render_mesh. */
int nmi_level_create_mesh(nmi_ctx *ctx, const float *d_xyz, const float *d_uv, int64_t n_triangles, const nmi_texture *tex,
                          const uint8_t *d_frame, int32_t S, int32_t Wn, nmi_level **out);
/* The same with a vertex-coloured mesh as the map: d_xyz / d_red as for nmi_render_mesh_colored, read in place (they must stay
 * valid and unchanged).  A mesh level in every other respect: the same graph (prep -> binning + warp workgroups -> clip ->
 * tiles -> search), and every nmi_level_* call below applies to it as to a textured one. */
int nmi_level_create_mesh_colored(nmi_ctx *ctx, const float *d_xyz, const float *d_red, int64_t n_triangles, const uint8_t *d_frame,
                                  int32_t S, int32_t Wn, nmi_level **out);
int nmi_level_run(nmi_level *lv, const float *h_mvps, const double *h_forward, int64_t *h_best_index, float *h_best_score);
/*
 * Level sharded over ranks (new; SURVEY.md 8e applied to the device-side level -- the LATENCY form of BASELINE.json configs[4]:
 * keyframes of a live sequence are not independent, each search is seeded from the drift since the previous NMI fix,
 * src/Tracking.cc:2001-2053, inside the sequential Track(), :598-616, so a live level can only be made faster by sharing ITS
 * candidates).  A _block level covers renders [s_offset, s_offset + S_local) x warps [w_offset, w_offset + Wn_local) of an
 * S_total x Wn_total level: the rank renders only its S_local views (h_mvps [S_local][16]), warps the frame Wn_local times
 * (h_forward [Wn_local][9]) and scores its cells with GLOBAL linear indices w * S_total + s.  Either count may be 0 (more
 * ranks than cells on the sharded axis): the rank then only takes part in the exchange.  nmi_level_run on a block returns
 * the block's own winner (for callers that reduce the keys themselves, e.g. torch.distributed over gloo: nmi_key_pack);
 * nmi_level_run_rccl adds the level's only exchange -- ncclAllReduce(ncclMax, ncclUint64) of the 8-byte key on the
 * context's stream, out of place -- and returns the level's winner on every rank.  Every rank of the communicator must
 * call it once per level.
 */
int nmi_level_create_block(nmi_ctx *ctx, const float *d_xyz, const float *d_red, int64_t n_points, const uint8_t *d_frame,
                           int32_t S_local, int32_t s_offset, int32_t S_total, int32_t Wn_local, int32_t w_offset, int32_t Wn_total,
                           float point_size, nmi_level **out);
int nmi_level_create_mesh_block(nmi_ctx *ctx, const float *d_xyz, const float *d_uv, int64_t n_triangles, const nmi_texture *tex,
                                const uint8_t *d_frame, int32_t S_local, int32_t s_offset, int32_t S_total, int32_t Wn_local,
                                int32_t w_offset, int32_t Wn_total, nmi_level **out);
int nmi_level_create_mesh_colored_block(nmi_ctx *ctx, const float *d_xyz, const float *d_red, int64_t n_triangles, const uint8_t *d_frame,
                                        int32_t S_local, int32_t s_offset, int32_t S_total, int32_t Wn_local, int32_t w_offset,
                                        int32_t Wn_total, nmi_level **out);
int nmi_level_run_rccl(nmi_level *lv, const float *h_mvps, const double *h_forward, void *nccl_comm, int64_t *h_best_index,
                       float *h_best_score);
/* Host copies of what the latest nmi_level_run produced: the S renders [S][H][W], the Wn warps [Wn][H][W] and the rating
 * table [Wn][S] (any pointer may be NULL).  Blocking; for tests and debugging (the reference's orb_prop_log dumps,
 * src/Tracking.cc:1911-1948, serve the same purpose). */
int nmi_level_copy_outputs(nmi_level *lv, uint8_t *h_renders, uint8_t *h_warps, float *h_ratings);
/*
 * Masked levels.  nmi_level_set_masks turns masks on (enabled = 1) or off (0) for a level made by any of the four
 * nmi_level_create* calls.  It captures the level's graph again and waits for a replay in flight.  Masked, every replay also
 * computes the warps' masks, exactly as nmi_warp_stack_masked does for the same homographies and d_frame_mask, and their
 * counts len_w, and scores with nmi_search_grid_masked's arithmetic (nmi_masked_grid_kernel, or the masked pixel-range
 * kernel for mid-size grids): same renders, same masks, same ratings, winner and score bits as those calls made one after
 * the other.  Blocks score their local warps with their own len_w and report global indices; empty blocks still take
 * part in the RCCL exchange.
 * d_frame_mask: uint8 [H][W], nonzero = usable, or NULL = border masks only.  Kept like d_frame: it must stay valid in
 * place; its CONTENTS may change between runs.  enabled = 0 restores the unmasked graph (d_frame_mask must then be NULL)
 * and frees the mask buffers.
 * Memory: a masked level owns its masks (Wn x H x W bytes), its counts and its per-warp term tables, Wn x (H x W + 1)
 * floats -- 44 MB for 27 warps at 848 x 480; both grow with Wn.  The tables are rebuilt only for the warps whose len_w
 * changed since the previous replay (within a strategy level the warps, hence the counts, repeat), and are never shared
 * with the standalone masked calls or with other levels.
 * nmi_level_run, nmi_level_run_rccl, nmi_level_copy_outputs keep their meaning on a masked level.
 */
int nmi_level_set_masks(nmi_level *lv, int32_t enabled, const uint8_t *d_frame_mask);
/* Host copies of the latest replay's warp masks [Wn][H][W] and counts [Wn] (either pointer may be NULL).  Blocking.
 * NMI_ERR_INVALID_ARGUMENT on a level without masks. */
int nmi_level_copy_masks(nmi_level *lv, uint8_t *h_warp_masks, int32_t *h_counts);
/*
 * Covered levels.  nmi_level_set_coverage turns coverage on (enabled = 1) or off (0) for a level made by any of the four
 * nmi_level_create* calls.  It captures the level's graph again and waits for a replay in flight, as nmi_level_set_masks
 * does.  Covered, every replay renders with coverage on the level's own render path (the renders stay byte-identical to the
 * unmasked level's; the masks are nmi_render_points_masked's / nmi_render_mesh_masked's), computes the warps' masks exactly
 * as nmi_warp_stack_masked does for the same homographies and d_frame_mask (NULL = border masks only), and scores with
 * nmi_search_grid_covered's arithmetic (the covered grid kernel, or the covered pixel-range kernel for mid-size grids):
 * ratings, winner index and score bits equal those of nmi_render_*_masked -> nmi_warp_stack_masked ->
 * nmi_search_grid_covered on the same inputs.  Blocks score their local candidates with their own len[w][s] and report
 * global indices; empty blocks still take part in the RCCL exchange.  d_frame_mask is kept like d_frame: it must stay valid
 * in place; its contents may change between runs.  enabled = 0 restores the unmasked graph (d_frame_mask must then be NULL)
 * and frees the coverage buffers.
 * A level is unmasked, masked or covered, never two at once: nmi_level_set_coverage on a masked level and
 * nmi_level_set_masks on a covered level return NMI_ERR_INVALID_ARGUMENT (for either value of enabled) and leave the level
 * as it was; nmi_level_copy_masks returns NMI_ERR_INVALID_ARGUMENT on a covered level.  A NULL level, enabled outside
 * {0, 1} or a mask passed with enabled = 0 are NMI_ERR_INVALID_ARGUMENT.
 * Memory: a covered level owns its render masks (S x H x W bytes), its warp masks (Wn x H x W bytes), len[w][s] (Wn x S
 * int32) and a redo list (Wn x S int32) -- no term tables: 22 MB for 27 + 27 at 848 x 480.  Never shared with the
 * standalone covered calls or with other levels.
 * nmi_level_run, nmi_level_run_rccl, nmi_level_copy_outputs keep their meaning on a covered level.
 */
int nmi_level_set_coverage(nmi_level *lv, int32_t enabled, const uint8_t *d_frame_mask);
/* Host copies of the latest replay's render masks [S][H][W], warp masks [Wn][H][W] and len [Wn][S] (any pointer may be
 * NULL).  Blocking.  NMI_ERR_INVALID_ARGUMENT on a level without coverage. */
int nmi_level_copy_coverage(nmi_level *lv, uint8_t *h_render_masks, uint8_t *h_warp_masks, int32_t *h_counts);
/*
 * Distorted lenses.  nmi_level_set_distortion(lv, K, dist) turns undistortion on for a level made by any of the four
 * nmi_level_create* calls: d_frame is then the RAW frame, and so is a d_frame_mask given to nmi_level_set_masks /
 * nmi_level_set_coverage.  Every replay runs one nmi_undistort_frame node after the prep node, into a frame (and, when the
 * level is masked or covered, a mask) the level owns; the warps, their masks and the search read those.  Ratings, winner
 * index and score bits equal the standalone chain's: nmi_undistort_frame(raw, NULL) -> nmi_warp_stack -> render ->
 * nmi_search_grid (plain); nmi_undistort_frame(raw, raw_mask) -> nmi_warp_stack_masked(ud, ud_mask) ->
 * nmi_search_grid_masked (masked), or the covered chain; nmi_level_copy_outputs' warps are those of the undistorted frame.
 * The call captures the graph again and waits for a replay in flight, as nmi_level_set_masks does; set and clear it in any
 * order with the masks and coverage, which keep it.  dist = NULL or five zero coefficients turn it off: the graph is again
 * the never-distorted level's, and the level frees its buffers (H x W bytes, and H x W more while masked or covered).  Empty blocks
 * take the setting and have no node.  NMI_ERR_INVALID_ARGUMENT (the level left as it was): a NULL level, K or dist as for
 * nmi_undistort_frame (K is not read when dist is NULL).
 */
int nmi_level_set_distortion(nmi_level *lv, const double K[9], const float dist[5] /* NULL = off */);
/*
 * Fisheye lenses.  nmi_level_set_distortion_fisheye is nmi_level_set_distortion for the model of nmi_undistort_frame_fisheye:
 * every replay's undistortion node is that call's, and the replay equals the same chains with it in nmi_undistort_frame's
 * place.  A level has one lens setting: of the two setters the later call wins, and dist = NULL in either turns it off.  Four
 * zero coefficients do not (an ideal equidistant lens is still a remap).  With nmi_level_set_frame_reduction, K and K_raw are
 * those of the reduced frame.  Everything else -- capturing again, waiting for a replay in flight, masks, coverage, frame
 * format and reduction in any order, empty blocks, the RCCL and block forms, the buffers freed when off, the errors with K_raw
 * (NULL = K) held to K's rules -- as nmi_level_set_distortion.
 */
int nmi_level_set_distortion_fisheye(nmi_level *lv, const double K[9], const double K_raw[9] /* NULL = K */,
                                     const float dist[4] /* NULL = off */);
/*
 * Colour and pitched frames.  nmi_level_set_frame_format(lv, format, pitch) makes a level of any of the four nmi_level_create*
 * forms (and its RCCL runs) read d_frame -- d_frame alone; a frame mask stays dense uint8 [H][W] in raw coordinates -- in place
 * on every replay as H rows of pitch bytes in format (pitch 0: dense).  The replay gains one node after the prep node, which
 * writes a grey frame the level owns (H x W bytes, 16-byte aligned: the fused front kernels stay eligible); with distortion on
 * it is the single node that converts and undistorts at once, with the bytes of the chain.  Ratings, winner index, score bits,
 * warps, masks and coverage equal the standalone chain's: nmi_gray_frame -> [nmi_undistort_frame] -> the level's chain on the
 * grey frame.  The call captures the graph again and waits for a replay in flight, as nmi_level_set_distortion does; set it in
 * any order with masks, coverage and distortion, which keep it.  (NMI_FRAME_GRAY, 0) or (NMI_FRAME_GRAY, W) turns it off: the
 * graph is again the never-formatted level's, and the level frees its grey frame.  Empty blocks take the setting and have no
 * node.  NMI_ERR_INVALID_ARGUMENT (the level left as it was): a NULL level, format or pitch as for nmi_gray_frame.
 */
int nmi_level_set_frame_format(nmi_level *lv, int32_t format, int64_t pitch /* bytes, 0 = dense */);
/*
 * Full-size frames.  nmi_level_set_frame_reduction(lv, factor, format, pitch) is nmi_level_set_frame_format with a factor: the
 * level (any of the four nmi_level_create* forms; plain, masked or covered) reads d_frame in place on every replay as f * H rows
 * of pitch bytes holding f * W pixels in format.  Factor 1 is that call exactly; of the two calls the later one wins, and
 * (1, NMI_FRAME_GRAY, 0) turns both off.  A frame mask (nmi_level_set_masks / _set_coverage) stays dense [H][W] at the search
 * size; with distortion set, K and the mask are those of the reduced frame (nmi_config_reduce gives that K).  Each replay equals
 * the standalone chain nmi_reduce_frame -> [nmi_undistort_frame] -> the level's chain on the grey frame: winner index and score
 * bits ==, warps, masks and counts byte-equal.  The graph takes one node that converts and reduces; with distortion a second
 * one, the undistortion node, reads the reduced frame from a buffer of the level's own (H x W bytes more).  Captures again and
 * waits for a replay in flight, as the other setters do; set it in any order with masks, coverage and distortion, which keep
 * it.  NMI_ERR_INVALID_ARGUMENT (the level left as it was): a NULL level, factor, format or pitch as for nmi_reduce_frame.
 */
int nmi_level_set_frame_reduction(nmi_level *lv, int32_t factor /* 1..4 */, int32_t format, int64_t pitch /* bytes, 0 = dense */);
/* The tone map of a GRAY16 frame ("Deep frames", above); the level's d_frame must then be 2-byte aligned.  NULL = the default. */
int nmi_level_set_tone_map(nmi_level *lv, const nmi_tone_map *tm);
/*
 * The valid range of a deep frame ("Deep frames", above: Valid range) as the level's own setting, like its tone map: 0 <= lo <=
 * hi <= 65535, (0, 65535) = off, the setting of every new level, under which the graph, every kernel launched, every buffer and
 * every output byte are what they are without this call.  nmi_set_valid_range does not reach a level.  The range is kept, and
 * ignored, under every frame format that is not deep; it applies to NMI_FRAME_GRAY16 and to every format that unpacks to it
 * (validity is taken on the container).
 *   Plain level        statistics only: the grey frame the warps read is nmi_gray_frame's / nmi_reduce_frame's under that range.
 *                      No mask is made.
 *   Masked or covered  also the frame mask the warp masks are made from: nmi_deep_frame's d_mask, 1 iff all f x f source pixels
 *                      are valid and the d_frame_mask given to nmi_level_set_masks / _set_coverage is nonzero there (NULL:
 *                      validity alone -- nmi_level_set_masks(lv, 1, NULL) plus a range is how a depth level says "validity
 *                      only").  Dense [H][W] at the search size, written by the same conversion node (its masked form, no extra
 *                      node) into a buffer of the level's own: the caller's d_frame_mask is only ever read.  With a lens set it
 *                      is the undistortion node's raw mask, and the warps read the undistorted one, exactly as a caller's raw
 *                      frame mask.
 * Each replay equals, on a context whose range and tone map are the level's, the standalone chain [nmi_unpack_frame] ->
 * nmi_deep_frame(src, pitch, f, d_frame_mask, gray, mask) -> [nmi_undistort_frame* (gray, mask)] -> nmi_warp_stack_masked -> the
 * renders -> nmi_search_grid_masked / _covered: winner index and score bits ==, rating table, warps, warp masks and counts
 * byte-equal.  A frame with no valid pixel: the global modes' table is all 0, the mask all 0, and the search is the masked
 * search's on all-zero warp masks.
 * Captures again and waits for a replay in flight, as the other setters do; set and clear it in any order with masks, coverage,
 * distortion (both models), frame format, reduction and tone map, which all keep it.  All six nmi_level_create* forms,
 * nmi_level_run and nmi_level_run_rccl; an empty block takes the setting and has no node.  Memory: H x W bytes more while the
 * range is on, the format is deep and the level is masked or covered; freed otherwise.
 * NMI_ERR_INVALID_ARGUMENT (the level left as it was): a NULL level, lo < 0, lo > hi, hi > 65535.
 */
int nmi_level_set_valid_range(nmi_level *lv, int32_t lo, int32_t hi /* 0 <= lo <= hi <= 65535; (0, 65535) = off */);

/*
 * Depth levels (new): a level whose renders are depth renders ("Depth maps" above: nmi_render_points_depth /
 * nmi_render_mesh_depth).  The shade is one more setting of the level: the render node of the captured graph shades from the
 * winners' depths, everything behind or beside it -- warps, masks, coverage, every intake setting, the search, nmi_level_run_rccl
 * -- is unchanged and unaware.  The coverage of a covered depth level is the depth shader's own mask.
 *   nmi_level_create_depth        a level of a map WITHOUT attributes: map_kind NMI_MAP_POINTS (d_xyz float [n][3], every point
 *                                 splats colour 0; point_size as nmi_level_create) or NMI_MAP_MESH (d_xyz float [3 n][3], n
 *                                 triangles; point_size ignored).  Otherwise nmi_level_create's arguments.
 *   nmi_level_create_depth_block  its block form: the block arguments of nmi_level_create_block.
 *   nmi_level_set_depth_shade     on ANY level -- cloud, textured mesh, coloured mesh, depth, block forms included: `shade` turns
 *                                 its renders into depth renders, NULL turns them back into the map's colour.  NULL on a level
 *                                 created without attributes is NMI_ERR_INVALID_ARGUMENT (it has no colour to go back to).
 * Each replay's renders equal nmi_render_points_depth's / nmi_render_mesh_depth's byte for byte (nmi_level_copy_outputs), its
 * coverage masks theirs (nmi_level_copy_coverage).  The depth-camera level is such a level plus nmi_level_set_frame_format(
 * NMI_FRAME_GRAY16), nmi_level_set_tone_map(NMI_TONE_WINDOW(lo, hi), 16 bits), nmi_level_set_valid_range(1, 65535) and
 * nmi_level_set_masks(1, NULL) or nmi_level_set_coverage(1, NULL), with the same (lo, hi) in the shade.
 * The setter captures again and waits for a replay in flight, as the other setters do; a refused or failed call leaves the level
 * as it was.  An empty block takes the setting and has no node.  Memory: a point-cloud level created here holds n floats of zeros
 * for the colours it does not have.
 * NMI_ERR_INVALID_ARGUMENT: a bad shade (as nmi_render_points_depth), a map_kind that is neither constant, the create forms' own
 * cases (nmi_level_create, nmi_level_create_block), a NULL level.
 */
#define NMI_MAP_POINTS 0
#define NMI_MAP_MESH 1
int nmi_level_create_depth(nmi_ctx *ctx, int32_t map_kind, const float *d_xyz, int64_t n, const uint8_t *d_frame, int32_t S, int32_t Wn,
                           float point_size, const nmi_depth_shade *shade, nmi_level **out);
int nmi_level_create_depth_block(nmi_ctx *ctx, int32_t map_kind, const float *d_xyz, int64_t n, const uint8_t *d_frame, int32_t S_local,
                                 int32_t s_offset, int32_t S_total, int32_t Wn_local, int32_t w_offset, int32_t Wn_total, float point_size,
                                 const nmi_depth_shade *shade, nmi_level **out);
int nmi_level_set_depth_shade(nmi_level *lv, const nmi_depth_shade *shade /* NULL = back to the map's colour */);
/*
 * Ranked peaks of a level ("Ranked peaks" below gives the rule).  nmi_level_set_peaks(lv, K, num, radius) with K in 1 .. 64 adds
 * the peaks kernel to the level's graph, as one more node on the main chain after the search, reading the level's rating table;
 * K = 0 takes it out again (num and radius may then be NULL).  A setting like every other: it captures the graph again, waits
 * for a replay in flight, works with masks, coverage and every intake setting, and a refused call leaves the level as it was.
 * nmi_level_run, its winner, its pinned word and its timing are the same with peaks on or off: the call returns at the winner,
 * and the peaks node runs behind it on the context's stream.
 * nmi_level_copy_peaks waits for the latest replay's peaks and copies the K keys (either pointer may be NULL, not both); h_count
 * receives the number of non-zero keys.  Before the first replay after nmi_level_set_peaks turned them on the keys are zeros.
 * NMI_ERR_INVALID_ARGUMENT: a NULL level, K outside 0 .. 64, with K > 0 a NULL num or radius, a count < 1, a negative radius, or
 * num[0] * num[1] * num[2] != S or num[3] * num[4] * num[5] != Wn of the level; nmi_level_copy_peaks on a level without peaks.
 * NMI_ERR_UNSUPPORTED: K > 0 on a block of a sharded level (greedy suppression over a block is not the suppression of the whole
 * grid), or on a level of more than 65,536 candidates.
 */
int nmi_level_set_peaks(nmi_level *lv, int32_t K, const int32_t num[6], const int32_t radius[6]);
int nmi_level_copy_peaks(nmi_level *lv, uint64_t *h_keys, int32_t *h_count);
/*
 * Refined peaks of a level ("Refined peaks" below gives the rule).  nmi_level_set_refine(lv, on) with on != 0 adds the refine
 * kernel to the level's graph, as one more node behind the peaks node, reading the keys that node wrote and the level's rating
 * table; on = 0 takes it out again, and so does nmi_level_set_peaks with K = 0.  A setting like every other (see
 * nmi_level_set_peaks): nmi_level_run, its winner, its pinned word and its timing are the same with it on or off.
 * nmi_level_copy_refined waits for the latest replay's records and copies the K of them (K as given to nmi_level_set_peaks;
 * either pointer may be NULL, not both); h_count receives the number of records with a key.  Before the first replay after
 * nmi_level_set_refine turned them on the records are zeros.
 * NMI_ERR_INVALID_ARGUMENT: a NULL level; nmi_level_set_refine on a level whose peaks are off; nmi_level_copy_refined on a level
 * without refined peaks.  NMI_ERR_UNSUPPORTED: a block of a sharded level, as for its peaks.
 */
int nmi_level_set_refine(nmi_level *lv, int32_t on);
int nmi_level_copy_refined(nmi_level *lv, nmi_refined_peak *h_records, int32_t *h_count);
int nmi_level_destroy(nmi_level *lv);

/*
 * Streaming form (BASELINE.json config 5): keyframes / search levels whose render stacks arrive from host memory.
 * A stream owns `depth` device slots; nmi_stream_submit enqueues, without blocking,
 *   copy stream    : hipMemcpyAsync of the pinned host render stack [S][H][W] (and the frame [H][W], if given) into a slot
 *   compute stream : (frame given) warp-stack production for h_forward [Wn][9]; the grid kernel; 8-byte winner -> pinned host
 * so the H2D copy of level i+1 overlaps the search of level i (the reference uploads and searches serially,
 * src/Tracking.cc:1871-1902).  Tickets complete in submission order.  nmi_stream_wait blocks on one ticket.
 * A slot is reused by submission i + depth only after ticket i was waited for.  h_* buffers must stay valid (and should be
 * page-locked, e.g. hipHostMalloc) until the ticket completes.  Passing h_frame == NULL re-uses the warp stack produced by
 * the most recent submission that had a frame.
 * A ticket whose small grid timed out in the split kernel (see nmi_create) is redone inside nmi_stream_wait when its warp
 * stack is still on the device; when a later frame has replaced it the wait returns NMI_ERR_NOT_READY, the ticket's rating
 * table is withheld (nmi_stream_copy_ratings fails) and the caller submits that level again.
 */
typedef struct nmi_stream nmi_stream;
int nmi_stream_create(nmi_ctx *ctx, int32_t max_S, int32_t max_Wn, int32_t depth, nmi_stream **out);
int nmi_stream_destroy(nmi_stream *st);
int nmi_stream_submit(nmi_stream *st, const uint8_t *h_render_stack, int32_t S, const uint8_t *h_frame,
                      const double *h_forward, int32_t Wn, int64_t *ticket);
/* Block form for a level sharded over ranks (see nmi_level_create_block): this rank uploads and scores only renders
 * [s_offset, s_offset + S_local) of the level's S_total (the H2D traffic that bounds the streamed form is divided by the
 * number of ranks) against warps [w_offset, w_offset + Wn_local) of Wn_total, which it makes locally from the frame;
 * h_forward holds the Wn_local homographies of its block.  With nccl_comm != NULL the key is MAX-all-reduced on the compute
 * stream right behind the search (every rank submits the levels in the same order) and the ticket completes with the
 * level's winner; with NULL it completes with the block's own key.  S_local may be 0 (h_render_stack may then be NULL). */
int nmi_stream_submit_block(nmi_stream *st, const uint8_t *h_render_stack, int32_t S_local, int32_t s_offset, int32_t S_total,
                            const uint8_t *h_frame, const double *h_forward, int32_t Wn_local, int32_t w_offset, int32_t Wn_total,
                            void *nccl_comm, int64_t *ticket);
int nmi_stream_wait(nmi_stream *st, int64_t ticket, int64_t *h_best_index, float *h_best_score);
/* Optional rating tables: after nmi_stream_keep_ratings(st, 1) every submission also stores its [Wn][S] table in its slot;
 * nmi_stream_copy_ratings copies the table of a ticket that has been waited for (n = Wn * S floats), valid until the
 * slot is submitted to again. */
int nmi_stream_keep_ratings(nmi_stream *st, int32_t enabled);
int nmi_stream_copy_ratings(nmi_stream *st, int64_t ticket, float *h_ratings, int64_t n);
/*
 * Masked and covered tickets: the stream's forms of nmi_search_grid_masked and nmi_search_grid_covered.  A ticket's winner
 * index, score bits, rating table (nmi_stream_keep_ratings) and counts are those of the standalone calls on the same inputs:
 *   masked   nmi_warp_stack_masked(frame, frame_mask, forward) followed by nmi_search_grid_masked;
 *   covered  the same warps and warp masks, the render masks unpacked from h_render_mask_bits (nmi_pack_mask_bits' layout,
 *            [S][ceil(H*W/8)], render layout), and nmi_search_grid_covered.
 * The _block forms report global indices exactly as nmi_stream_submit_block does, their cells equal the whole grid's cells,
 * and with nccl_comm the key is MAX-all-reduced right behind the search; empty blocks (S_local == 0) still take part.
 *   h_frame_mask  uint8 [H][W], nonzero = usable, uploaded with the frame on the copy stream; NULL = border masks only.  A
 *                 frame mask without a frame is NMI_ERR_INVALID_ARGUMENT.
 *   h_frame NULL  reuses the warps AND warp masks of the most recent frame submission; when that was a plain nmi_stream_submit*
 *                 (which makes no masks) the call is NMI_ERR_INVALID_ARGUMENT.  A plain frame-less ticket after a masked or
 *                 covered frame is fine (the warp stack is byte-identical).
 *   h_render_mask_bits  must stay valid until the ticket completes, like h_render_stack; NULL with S > 0 is
 *                 NMI_ERR_INVALID_ARGUMENT.  The bits cross PCIe (+12.5 % on the render stack) and are unpacked on the device.
 * One stream carries any mix of plain, masked and covered tickets; they complete in submission order.  Masked and covered
 * tickets never use the split kernel, so nmi_stream_wait never returns NMI_ERR_NOT_READY for them; mid-size grids take the
 * masked / covered pixel-range kernel by the standalone calls' rules (those heal inside the launch).  They leave
 * nmi_last_mask_counts / nmi_last_cover_counts reporting the latest standalone search.
 * Memory, allocated on the stream's first masked or covered submission (never for a plain-only stream): 2 x H*W (frame masks)
 * + 2 x max_Wn x H*W (warp masks) + (depth + 1) x max_S x max_Wn x 4 bytes (counts, redo list); on the first masked one also
 * 2 x max_Wn x (H*W + 1) x 4 bytes (term tables: 88 MB at 27 warps and 848 x 480) + 2 x max_Wn x 4; on the first covered one
 * depth x max_S x ceil(H*W/8) (bits) + max_S x H*W (one unpacked render-mask buffer shared by all slots).
 * nmi_stream_copy_counts: len_w [Wn] of a masked ticket, len[w][s] [Wn][S] of a covered ticket (n must be exactly that);
 * valid from nmi_stream_wait until the slot is reused.  NMI_ERR_INVALID_ARGUMENT on a plain ticket.
 */
int nmi_stream_submit_masked(nmi_stream *st, const uint8_t *h_render_stack, int32_t S, const uint8_t *h_frame,
                             const uint8_t *h_frame_mask /* nullable */, const double *h_forward, int32_t Wn, int64_t *ticket);
int nmi_stream_submit_masked_block(nmi_stream *st, const uint8_t *h_render_stack, int32_t S_local, int32_t s_offset, int32_t S_total,
                                   const uint8_t *h_frame, const uint8_t *h_frame_mask /* nullable */, const double *h_forward,
                                   int32_t Wn_local, int32_t w_offset, int32_t Wn_total, void *nccl_comm, int64_t *ticket);
int nmi_stream_submit_covered(nmi_stream *st, const uint8_t *h_render_stack, const uint8_t *h_render_mask_bits, int32_t S,
                              const uint8_t *h_frame, const uint8_t *h_frame_mask /* nullable */, const double *h_forward,
                              int32_t Wn, int64_t *ticket);
int nmi_stream_submit_covered_block(nmi_stream *st, const uint8_t *h_render_stack, const uint8_t *h_render_mask_bits, int32_t S_local,
                                    int32_t s_offset, int32_t S_total, const uint8_t *h_frame, const uint8_t *h_frame_mask /* nullable */,
                                    const double *h_forward, int32_t Wn_local, int32_t w_offset, int32_t Wn_total, void *nccl_comm,
                                    int64_t *ticket);
int nmi_stream_copy_counts(nmi_stream *st, int64_t ticket, int32_t *h_counts, int64_t n);
/*
 * Distorted lenses on a stream: after nmi_stream_set_distortion(st, K, dist) every frame submission, of every kind (plain,
 * masked, covered and their _block forms), takes h_frame and h_frame_mask as RAW: the frame is undistorted on the compute
 * stream before its warps (nmi_undistort_frame, into a pair of frames -- and, for masked and covered frames, masks -- beside
 * the uploaded ones), and a ticket equals the chain nmi_level_set_distortion names.  Tickets submitted before the call are
 * not affected; frame-less tickets reuse the most recent warps as always.  dist = NULL or five zero coefficients turn it off:
 * later tickets are those of a stream that never had it.  NMI_ERR_INVALID_ARGUMENT as for nmi_level_set_distortion (the
 * stream left as it was).  Memory: 2 x H*W bytes on the first distorted frame, 2 x H*W more on the first masked or covered one.
 */
int nmi_stream_set_distortion(nmi_stream *st, const double K[9], const float dist[5] /* NULL = off */);
/* Fisheye lenses on a stream: nmi_stream_set_distortion for the model of nmi_undistort_frame_fisheye.  One lens setting per
 * stream: of the two setters the later call wins, dist = NULL in either turns it off, four zero coefficients do not. */
int nmi_stream_set_distortion_fisheye(nmi_stream *st, const double K[9], const double K_raw[9] /* NULL = K */,
                                      const float dist[4] /* NULL = off */);
/*
 * Colour and pitched frames on a stream: after nmi_stream_set_frame_format(st, format, pitch) every frame submission, of every
 * kind (plain, masked, covered and their _block forms), reads h_frame as H rows of pitch bytes in format (pitch 0: dense).  The
 * frame crosses to the device with hipMemcpy2DAsync into a dense colour slot (a pair: frames alternate) and is converted on the
 * compute stream before its warps -- in one node with the undistortion when that is on -- and a ticket equals a grey ticket on
 * nmi_gray_frame's frame.  Frame masks (h_frame_mask) stay dense [H][W].  Tickets submitted before the call are not affected;
 * frame-less tickets reuse the most recent warps as always.  (NMI_FRAME_GRAY, 0) or (NMI_FRAME_GRAY, W) turns it off.
 * NMI_ERR_INVALID_ARGUMENT as for nmi_level_set_frame_format (the stream left as it was).  Memory: 2 x H*W*bytes per pixel on the
 * first formatted frame, and 2 x H*W for the grey frames unless undistortion already holds them.
 */
int nmi_stream_set_frame_format(nmi_stream *st, int32_t format, int64_t pitch /* bytes, 0 = dense */);
/*
 * Full-size host frames on a stream: nmi_stream_set_frame_reduction is nmi_stream_set_frame_format with a factor (factor 1 is
 * that call; the later of the two wins; (1, NMI_FRAME_GRAY, 0) turns both off).  After it every frame submission of every kind
 * reads h_frame as f * H rows of pitch bytes holding f * W pixels in format.  The frame crosses with hipMemcpy2DAsync into a
 * dense full-size slot (a pair) and is reduced on the compute stream before the warps (and before the undistortion when that is
 * on: two nodes); a ticket equals a grey ticket on nmi_reduce_frame's frame.  Frame masks stay [H][W].  Tickets submitted before
 * the call are not affected.  NMI_ERR_INVALID_ARGUMENT as for nmi_level_set_frame_reduction (the stream left as it was).
 * Memory: 2 x f^2 * W*H * bytes per pixel on the first such frame, and 2 x H*W for the grey frames unless undistortion already
 * holds them.
 */
int nmi_stream_set_frame_reduction(nmi_stream *st, int32_t factor /* 1..4 */, int32_t format, int64_t pitch /* bytes, 0 = dense */);
/* The tone map of GRAY16 host frames ("Deep frames", above), for later submissions.  NULL = the default. */
int nmi_stream_set_tone_map(nmi_stream *st, const nmi_tone_map *tm);
/*
 * The valid range of deep host frames (nmi_level_set_valid_range's rule), the stream's own setting, for later submissions of
 * every kind: plain, masked, covered and their _block forms.  A plain ticket takes the statistics only.  A masked or covered
 * ticket's frame mask is nmi_deep_frame's d_mask -- validity ANDed with h_frame_mask, NULL: validity alone -- made on the device
 * by the frame's conversion, in place in the stream's frame-mask slot, so a depth stream uploads no H x W mask per keyframe; with
 * a lens set it is undistorted like an uploaded raw mask.  A ticket equals the same submission on a plain-grey stream given
 * nmi_deep_frame's grey frame and mask.  Tickets already submitted are not affected; frame-less tickets reuse the latest warps
 * and warp masks as always.  (0, 65535) = off, the setting of every new stream; kept, and ignored, under every format that is not
 * deep.  Memory: none beyond the frame-mask pair a masked or covered stream already owns.
 * NMI_ERR_INVALID_ARGUMENT (the stream left as it was): a NULL stream, lo < 0, lo > hi, hi > 65535.
 */
int nmi_stream_set_valid_range(nmi_stream *st, int32_t lo, int32_t hi /* 0 <= lo <= hi <= 65535; (0, 65535) = off */);

/* Packed-key helpers (host side, pure). */
uint64_t nmi_key_pack(float score, int64_t global_linear_index);
int nmi_key_unpack(uint64_t key, int64_t *global_linear_index, float *score);

/*
 * Ranked peaks.  The K best SEPARATED candidates of a rating table, on the device: is the winner ambiguous (a second pose,
 * away from it, that scores almost as well), and which few poses are worth a finer level.  (New: the reference takes
 * find_max_elements(...)[0], helperFunctions.cpp:50-103, src/Tracking.cc:1905, and nothing else of the table.)
 *
 * Inputs.  A rating table float [Wn][S] (nmi_search_grid's d_ratings, a level's table); the six axis counts num[6] in the axis
 * order of nmi_host.h, S = num[0] * num[1] * num[2], Wn = num[3] * num[4] * num[5], the linear index nmi_sk_linear_index's
 * (axis 0 fastest); K in 1 .. 64; a per-axis radius[6], every entry >= 0.
 * Selection.  A cell qualifies when nmi_key_pack(score, index) != 0: negative scores (other than -0.0, which counts as 0.0) and
 * NaN never do.  Peak 0 is the qualifying cell with the greatest key.  Peak j is the qualifying cell with the greatest key that
 * is not inside the box of any of peaks 0 .. j - 1.  A cell is inside the box of peak p when |a_cell - a_p| <= radius[a] on all
 * six axes, in axis coordinates: the box is clipped at the grid's edges and does not wrap (a cell that is linearly adjacent
 * across a row end is no neighbour).  Selection stops after K peaks, or when no qualifying cell is left.
 * Output.  The peaks' keys, uint64 [K], in rank order (nmi_key_unpack gives index and score); entries from `count` onward are
 * 0; count = the number of peaks found.
 * Everything is compares on integers and float bits: the device, nmi_find_peaks (nmi_host.h) and any model agree on every bit.
 * With radius all zero this is a plain top-K.  Peak 0 is the winner nmi_search_grid reports for the same table.
 *
 * nmi_rank_peaks is enqueued on the context's stream, after whatever wrote d_ratings there: one launch of one workgroup
 * (nmi_peaks.hip).  d_keys (device, uint64 [K]) and h_keys (host, uint64 [K]) may each be NULL, not both.  With h_keys the call
 * blocks until the keys are there, and h_count (nullable) receives the number of non-zero keys; without h_keys it only enqueues
 * and h_count is not written.
 * NMI_ERR_INVALID_ARGUMENT, before anything is enqueued and with the outputs untouched: a NULL context, table, num or radius, a
 * count < 1, K outside 1 .. 64, a negative radius, both outputs NULL.  NMI_ERR_UNSUPPORTED, likewise: a table of more than
 * 65,536 cells (one workgroup keeps the table in its registers; a form of several launches is not provided).
 * Not provided either: peaks of a keyframe stream's tickets, of sharded searches and blocks (greedy suppression over a block is
 * not that of the whole grid) and of the RCCL forms.  Sub-cell interpolation of a peak is "Refined peaks", next.  The strategy
 * driver (nmi_relocalize_with_strategy) is unchanged: it goes by the single winner.
 */
int nmi_rank_peaks(nmi_ctx *ctx, const float *d_ratings, const int32_t num[6], int32_t K, const int32_t radius[6],
                   uint64_t *d_keys /* nullable */, uint64_t *h_keys /* nullable: enqueue only */, int32_t *h_count /* nullable */);

/*
 * Refined peaks.  The quadratic through the 3 x ... x 3 neighbourhood of a peak of a rating table, on the device: the pose between
 * the cells (a level's worth of precision without rendering, warping or scoring anything), the interpolated score, and the
 * Hessian -- how sharp the optimum is on each axis and how the axes trade off, which is what tells an ambiguous search from a flat
 * one and what a back end wants as the weight of a relocalisation.  (New: the reference reaches finer poses only by halving the
 * step, src/Tracking.cc:2088-2130, and fixes NMI keyframes in BA with no weight, src/Optimizer.cc:82,548.)
 *
 * Inputs.  A rating table float [Wn][S]; num[6], axis order and linear index as for "Ranked peaks"; K keys, 1 <= K <= 64, as
 * nmi_rank_peaks writes them.  Output.  K records nmi_refined_peak (nmi_refined_peak.h, 152 bytes), record k for key k.
 * For a record, c is the cell of the key's index, f0 the table's value at c, f(c + ...) the table's value at a neighbour; the
 * score bits of the key are copied and not used.  A sample is USABLE when it is >= 0 (so -0.0 is) and finite: "qualifies" of the
 * peaks rule, plus finiteness.  All arithmetic is fp32, one rounding per operation, in the order written here.
 *  1. Empty record.  A key of 0, or an index that is not below the number of cells: every byte 0 but flags = NMI_REFINE_EMPTY.
 *     The table is not read for it.
 *  2. Unusable centre (+inf, for a key nmi_rank_peaks wrote).  key as given, score = f0, flags = NMI_REFINE_NONFINITE, all else 0.
 *  3. Active axes.  Axis a is active when 1 <= c_a <= num[a] - 2 and both f(c + e_a) and f(c - e_a) are usable.  num[a] == 1: no
 *     flag.  c_a on the first or last cell of an axis with num[a] >= 2: NMI_REFINE_BORDER(a), and no neighbour on that axis is
 *     looked at.  Else an unusable axial neighbour: NMI_REFINE_HOLE(a).  Offset, gradient and Hessian entries of an inactive axis
 *     are 0; no sample is ever taken outside the grid or across a row end.
 *  4. Gradient and diagonal of an active axis, f+ = f(c + e_a), f- = f(c - e_a):  g_a = 0.5f * (f+ - f-),
 *     H_aa = (f+ - f0) + (f- - f0).
 *  5. Cross terms of active axes a < b, f+- = f(c + e_a - e_b) and so on:  H_ab = 0.25f * ((f++ - f+-) - (f-+ - f--)).  If one of
 *     the four is unusable, H_ab = 0 and NMI_REFINE_CROSS_HOLE is set.  A record reads at most 1 + 12 + 60 = 73 samples.
 *  6. Coupled step.  With at least one active axis, A = -H on the active axes (A_ab = -H_ab) is factored as L D L^T without a
 *     square root, the pivots in axis order, j ascending over the active axes, k < j and i > j over the active axes, k ascending:
 *       d_j = A_jj - sum_k (L_jk * d_k) * L_jk        (v = A_jj; v = v - (L_jk * d_k) * L_jk for each k)
 *       d_j > 0, or the coupled step is not accepted (NaN is not > 0)
 *       L_ij = (A_ij - sum_k (L_ik * d_k) * L_jk) / d_j
 *     then A x = g:  z_i = g_i - sum_{k < i} L_ik * z_k, i ascending;  x_i = z_i / d_i - sum_{k > i} L_ki * x_k, i descending, each
 *     sum subtracted term by term, k ascending.  The step is accepted when every pivot passed and every -1 <= x_a <= 1: the offset
 *     is x and NMI_REFINE_COUPLED is set.  The bound of 1 means that the step interpolates inside the stencil and never extrapolates.
 *  7. Separable step, when the coupled step is not accepted: each active axis on its own.  H_aa < 0: offset_a = (-g_a) / H_aa,
 *     clamped to [-1, 1]; otherwise offset_a = 0 and NMI_REFINE_FLAT(a) is set.
 *  8. Score, the sums over the active axes in axis order, each from 0:
 *       score = (f0 + sum_a g_a * o_a) + 0.5f * sum_a o_a * (sum_b H_ab * o_b).
 * gradient and hessian (upper triangle, row-major) are those of items 4 and 5 whichever step was taken.
 * Overflow.  Usable samples are finite and >= 0, so every single difference of two samples is finite; the sums of item 4's and
 * item 5's differences can overflow to +-inf when samples are near the top of fp32's range (NMI scores are below 2).  The offsets
 * are in [-1, 1] even then -- a coupled x that is NaN fails its bound, and the separable quotient of a finite g_a by a negative or
 * infinite H_aa is never NaN -- but the score of item 8 can be NaN (0 * inf), and the Hessian holds the infinities.
 * The order of every operation is fixed by the numpy model tests/helpers/refine_np.py (float32 scalars), which is the executable
 * statement of this rule: the device, nmi_refine_peaks_host (nmi_host.h) and the model agree on every bit of every record.
 *
 * nmi_refine_peaks is enqueued on the context's stream, after whatever wrote d_ratings (and d_keys) there: one launch of K
 * workgroups of one wavefront each (nmi_refine.hip).  Exactly one of d_keys (device, uint64 [K]) and h_keys (host, uint64 [K]) is
 * non-NULL; host keys travel in the launch's arguments and are read before the call returns.  d_out (device) and h_out (host),
 * nmi_refined_peak [K] each, may each be NULL, not both.  With h_out the call blocks until the records are there; without it the
 * call only enqueues.
 * NMI_ERR_INVALID_ARGUMENT, before anything is enqueued and with the outputs untouched: a NULL context, table or num, a
 * count < 1, K outside 1 .. 64, both keys pointers or neither, both outputs NULL.  NMI_ERR_UNSUPPORTED, likewise: a table
 * whose indices do not fit the 32 bits a key has for them (2^32 - 1 cells or more).  The 65,536-cell limit of nmi_rank_peaks does
 * not apply: this kernel only gathers.
 * Not provided: refined peaks of a keyframe stream's tickets, of sharded searches and blocks and of the RCCL forms; moving a peak
 * to a neighbouring cell and fitting again (the bound of 1 and the clamp are the rule).  The strategy driver
 * (nmi_relocalize_with_strategy) is unchanged and still goes by whole cells; nmi_calculate_relocalization_offset and
 * nmi_refined_covariance (nmi_host.h) turn a record into a pose and a covariance for a caller who wants them.
 */
int nmi_refine_peaks(nmi_ctx *ctx, const float *d_ratings, const int32_t num[6], const uint64_t *d_keys /* or */,
                     const uint64_t *h_keys, int32_t K, nmi_refined_peak *d_out /* nullable */,
                     nmi_refined_peak *h_out /* nullable: enqueue only */);

/*
 * RCCL form: nmi_search_grid_shard / _block followed by ncclAllReduce(ncclMax, ncclUint64) of the key on the context's
 * stream over `nccl_comm` (an ncclComm_t created by the caller), then the 8-byte read-back.  A rank whose block is
 * empty (S_local == 0 or Wn_local == 0: fewer renders than ranks on a render-sharded level) contributes "no candidate"
 * and still takes part in the collective.  The _block form shards either axis (see nmi_search_grid_block).
 */
int nmi_search_grid_rccl(nmi_ctx *ctx, const uint8_t *render_stack, int32_t S_local, int32_t s_offset,
                         int32_t S_total, const uint8_t *warp_stack, int32_t Wn, float *d_ratings,
                         void *nccl_comm, int64_t *h_best_index, float *h_best_score);
int nmi_search_grid_block_rccl(nmi_ctx *ctx, const uint8_t *render_stack, int32_t S_local, int32_t s_offset, int32_t S_total,
                               const uint8_t *warp_stack, int32_t Wn_local, int32_t w_offset, int32_t Wn_total, float *d_ratings,
                               void *nccl_comm, int64_t *h_best_index, float *h_best_score);

/* Communicator bootstrap for hosts that have no ncclComm_t yet: rank 0 calls nmi_rccl_unique_id and
 * ships the 128 bytes to the other ranks by any means; every rank then calls nmi_rccl_comm_init. */
int nmi_rccl_unique_id(uint8_t out_id[128]);
int nmi_rccl_comm_init(nmi_ctx *ctx, const uint8_t id[128], int32_t rank, int32_t nranks, void **out_comm);
int nmi_rccl_comm_destroy(void *nccl_comm);

/*
 * Timing of the dominant kernel with HIP events on the context's stream.  When enabled, every grid /
 * pair launch is bracketed by hipEventRecord; nmi_last_kernel_ms returns the duration of the most
 * recent launch (synchronises on the stop event).
 */
int nmi_set_profiling(nmi_ctx *ctx, int32_t enabled);
int nmi_last_kernel_ms(nmi_ctx *ctx, float *h_ms);

/*
 * Tuning / ablation knobs (defaults are the shipped configuration; results stay exact for every value
 * except NMI_OPT_HIST_VARIANT = 2, which skips the counter-wrap bookkeeping, and a partial phase mask).
 */
#define NMI_OPT_HIST_VARIANT 1 /* 3 optimistic + verify + exact redo (default), 1 exact wrap bookkeeping throughout.  The
                                  experiments 0 (per-pixel wrap test), 2 (unchecked) and 4 (histogram and decode overlapped by
                                  wavefront role; exact but slower, profiles/NOTES.md) exist only in a library built with
                                  -DNMI_BUILD_ABLATIONS (NMI_ERR_UNSUPPORTED otherwise). */
#define NMI_OPT_PHASE_MASK 2   /* bit 0 histogram phase, bit 1 decode + score, bit 2 disable the flat-chunk shortcut; default 3.
                                  Bit 9 (tests): one part of the split kernel withholds its hand-off, so the bounded wait (2 ms) of
                                  the scoring workgroup times out and the call is redone by the one-workgroup kernel. */
#define NMI_OPT_WORKGROUPS 3   /* workgroups per launch; 0 = one per compute unit (default) */
#define NMI_OPT_RESULT_PATH 4  /* how the 8-byte winner reaches the host: 1 the kernel posts it to pinned host memory
                                  and the call polls it (default), 0 hipMemcpyAsync + hipStreamSynchronize */
#define NMI_OPT_XCD_TILING 5   /* 1 (default): candidates are visited in (warp x render) tiles so that the 32 workgroups
                                  of one XCD share ~12 images in its L2; 0: linear order.  Same results either way. */
#define NMI_OPT_TILE_QUEUE 6   /* mesh renderer: usable entries of each screen-tile bin (at most 255, the default; the value is
                                  clamped).  A triangle that finds a bin full is rasterised by its own lane instead; 0 = every
                                  triangle is.  Same image for every value (small values exercise the overflow path in tests). */
#define NMI_OPT_CLIP_QUEUE 11  /* mesh renderer: capacity of the queue that hands (triangle, view) pairs crossing the near plane to
                                  the clipping pass, at most 262144 (default).  With more such pairs than that the clipping
                                  pass finds them again itself; same image for every value (0 exercises that path in tests). */
#define NMI_OPT_SPLIT 7        /* small grids (nmi_eval_pair, collapsed search levels): K workgroups per candidate, each owning
                                  256 / K rows of the joint histogram, optionally x P pixel ranges (NMI_OPT_SPLIT_PIXELS);
                                  bit-identical results.  -1 (default, on 256 compute units): 8 x 4 up to 8 candidates, 8 x 2
                                  up to 16, 4 x 2 up to 32; 33 ... 128 candidates: 1 x P, pixel ranges only (nmi_pix_status; P = 4
                                  up to 64 candidates, 3 up to 85, 2 up to 128); none for larger grids; 0: never; 2 / 4 / 8: that
                                  K whenever the grid fits; 1: pixel ranges only, NMI_OPT_SPLIT_PIXELS = 2 ... 5 of them, whenever
                                  the grid fits. */
#define NMI_OPT_WAIT_MODE 8    /* how a blocking call waits for the posted result: 0 (default) spins on the pinned word
                                  (lowest latency, occupies the calling core for the search), 1 yields the core between
                                  polls (sched_yield; for hosts whose other threads need the core, e.g. ORB-SLAM2's
                                  LocalMapping / LoopClosing).  NMI_OPT_RESULT_PATH 0 sleeps in hipStreamSynchronize instead. */
#define NMI_OPT_SPLIT_PIXELS 10 /* additionally cut the pixels of each pair into 2 or 4 ranges (one workgroup per row part and
                                  range, merged per row part: nmi_eval_pair = 8 x 4 = 32 workgroups; 4 with 8 row parts only).
                                  -1 (default): see NMI_OPT_SPLIT; 1: never; 2 / 4: that many when it exists and fits
                                  (NMI_OPT_SPLIT 1: 2 ... 5). */
#define NMI_OPT_CONTENT_PATH 12 /* frames with few distinct intensities (posterised, thresholded, quantised): -1 (default)
                                  automatic -- every search by the general kernel also counts the distinct intensities (bins) its
                                  candidates' marginal histograms hold, (nr, nw), at no extra launch, and every few-levels search
                                  probes its two stacks; while nr * nw <= NMI_OPT_FEWLEVELS_BINS searches go down the few-levels
                                  path (rank images + 32-bit replicated counters; csrc/nmi_fewlevels_kernel.hip; with fewer than
                                  256 bins the background rule must be on).  A change of content costs one search on the slower
                                  path either way.  0: never; 1: always try it first.  Every few-levels search falls back to the
                                  general kernel on the device when its stacks do not qualify: results never depend on it. */
#define NMI_OPT_FEWLEVELS_BINS 13 /* largest nr * nw sent down the few-levels path (1..4096, default 4096) */
#define NMI_OPT_PIX_OWNER_BIAS 14 /* pixel-range kernel (nmi_pix_status): pixels a candidate's owner adds beyond an equal share of the
                                  pair while its helpers' counters travel to it (default 49152 = 3.4 us of one CU's histogram
                                  phase); a matter of speed only */
#define NMI_OPT_STAMPS 9       /* profiling tools only: value = device pointer to uint64 [workgroups][8]; workgroups of the
                                  split kernel store wall-clock stamps (100 MHz) at their phase boundaries there; 0 = off */
#define NMI_OPT_STAMP_CANDIDATE 15 /* profiling tools only: the stamped nmi_grid_kernel (NMI_OPT_STAMPS on a grid search) stamps
                                  every workgroup's k-th candidate, k = value (default 0: its first).  Waits for the stream. */
#define NMI_OPT_WAVE_SHARES 16 /* profiling tools only: value = host pointer to uint32 [2][17], the cumulative shares (x 65536; 0
                                  first, 65536 last, never falling) of a candidate's pixels that the 16 wavefronts of the stamped
                                  nmi_grid_kernel take -- row 0 for a workgroup's first candidate, row 1 for its later ones.  The
                                  product's kernels keep their built-in shares (csrc/nmi_grid_device.h).  Waits for the stream. */
int nmi_set_option(nmi_ctx *ctx, int32_t option, int64_t value);

/* Split-kernel liveness (see nmi_create): *timeouts = hand-off timeouts so far, *cooldown_calls_left = small-grid launches
 * that will still go through the one-workgroup kernel before the split forms are tried again, *next_cooldown = length of
 * the pause the next timeout would start, *last_launch_parts = row parts per candidate of the most recent launch (0: the
 * one-workgroup kernel scored it).  Any pointer may be null.  Does not wait. */
int nmi_split_status(nmi_ctx *ctx, int32_t *timeouts, int32_t *cooldown_calls_left, int32_t *next_cooldown, int32_t *last_launch_parts);
/* Mid-size grids (33 ... 128 candidates on 256 compute units: the live strategy's collapsed-axis levels, Tracking.cc:2014-2043,
 * and a rank's share of a sharded 729-candidate grid) are scored by P workgroups per candidate, each adding a range of the
 * pair's PIXELS into a histogram of its own (csrc/nmi_pix_kernel.hip); bit-identical results; no residence condition, so
 * enqueue-only calls use it too.  *last_launch_ranges = P of the most recent launch (0: another kernel scored it);
 * *healed = candidates so far that their owner scored once more, alone, inside the launch -- nothing for the host to redo.
 * What it counts depends on the form: plain searches add the candidates whose owner gave up waiting for a helper (2 ms)
 * and nothing else; masked and covered searches add those AND the candidates whose merged counters failed the count test
 * (a 16-bit field wrapped).  nmi_pix_heal_counts tells the two causes apart for every form.  Waits for the context's
 * stream when healed is asked for.  Any pointer may be null. */
int nmi_pix_status(nmi_ctx *ctx, int32_t *last_launch_ranges, int32_t *healed);
/* The two causes of such a heal, candidates so far on this context, over plain, masked and covered searches alike (those
 * inside captured levels and stream tickets included): *timeouts = owners that gave up waiting for a helper; *count_test =
 * merged decodes whose total was not the number of pixels added (W*H / the masked pixels / the covered pixels): a wrapped
 * 16-bit field -- or, on content that cannot wrap one, a hand-off that was read stale.  Waits for the context's stream.
 * Any pointer may be null. */
int nmi_pix_heal_counts(nmi_ctx *ctx, int32_t *timeouts, int32_t *count_test);

/* Introspection. */
/* Copies the context's per-count term table, term[c] = (c/len) * log2(c/len) in the reference's fp32 form with
 * len = width * height (ComputeEntropyKernel, NMI.cu:242-263; term[0] = 0), c = 0..len, to host memory.
 * n must be width * height + 1.  Blocking.  Lets a test compare every entry with its oracle. */
int nmi_copy_term_table(nmi_ctx *ctx, float *h_out, int64_t n);
int nmi_abi_version(void);
const char *nmi_error_string(int code);
const char *nmi_last_error_detail(nmi_ctx *ctx); /* text of the last failing HIP/RCCL call, or "" */
int nmi_get_info(nmi_ctx *ctx, int32_t *compute_units, int32_t *workgroups_per_launch, int32_t *lds_bytes);
/* How the most recent search was scored (waits for it): *few_levels = 1 if it was sent down the few-levels path
 * (NMI_OPT_CONTENT_PATH) AND stayed there (the device's own verdict, read back), 0 if the general kernel scored it; *nr, *nw = distinct intensities the most
 * recent probe found in a render / warp stack (0, 0 before the first probe).  Any pointer may be null.  Diagnostics. */
int nmi_last_content(nmi_ctx *ctx, int32_t *few_levels, int32_t *nr, int32_t *nw);

#ifdef __cplusplus
}
#endif
#endif /* NMI_HIP_H */
