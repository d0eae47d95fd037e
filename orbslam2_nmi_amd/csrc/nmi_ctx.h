// nmi_ctx.h -- internal: the context object behind include/nmi_hip.h and the helpers its translation units share
// (nmi_capi.cpp: context + search; nmi_capi_producers.cpp: warp / render producers; nmi_capi_pipeline.cpp: captured level
// and streaming pipeline; nmi_capi_intake.cpp: the frame's way into both; nmi_capi_rccl.cpp: the RCCL entry points).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <new>
#include <string>
#include <vector>

#include "nmi_hip.h"
#include "nmi_covered.h"
#include "nmi_kernels.h"
#include "nmi_masked.h"
#include "nmi_mem.h"
#include "nmi_search_plan.h"
#include "nmi_tone.h"

// What a search launched (enqueue_grid, enqueue_grid_mask): the split-timeout redo logic and the status getters go by it.
struct SearchLaunch {
    nmi::SearchKernel kind = nmi::SearchKernel::none;
    int parts = 0;       // row parts per candidate (0 = not the row-split kernel)
    int pix = 0;         // pixel ranges per candidate when it was a pixel-range kernel (0 = it was not)
    uint32_t epoch = 0;  // its split epoch (meaningful when parts != 0)
    int few = 0;         // it went down the few-levels path (it may have fallen back)
};

using nmi_mem::DeviceBuffer;
using nmi_mem::PinnedBuffer;

// The mesh renderer's work area (nmi_render_mesh, a mesh level): the buffers, and the view of them nmi_mesh.hip takes.
struct MeshWorkArea {
    DeviceBuffer zbuf, bins, state, clip_queue, clip_state, pairs, pair_state;
    nmi::MeshWork view;
};

struct nmi_ctx {
    nmi_params params{};
    int device = 0;
    int compute_units = 0;
    int npix = 0;
    int shift = 0;
    nmi_mem::Stream own_stream;
    hipStream_t stream = nullptr;
    DeviceBuffer table;                    // float [npix + 1]
    DeviceBuffer d_keys;                   // unsigned long long [2]: device slots for the packed winner, used alternately (ping-pong)
    PinnedBuffer h_key;                    // unsigned long long: pinned host mirror (copy path)
    DeviceBuffer d_done;                   // unsigned int: finished-workgroup counter
    PinnedBuffer mailbox;                  // nmi::Mailbox, fine-grained: the kernel posts the winner here
    unsigned int seq = 0;                  // launches that post to the mailbox so far (blocking calls only)
    int slot = 0;                          // key slot of the next launch
    int last_slot = 0;                     // key slot of the most recent launch
    SearchLaunch last;                     // the most recent launch (written by commit_launch only)
    int pix_owner_bias = 49152;            // NMI_OPT_PIX_OWNER_BIAS: pixels the owner of a candidate adds beyond an equal share
    DeviceBuffer d_pix_timeouts;           // uint32_t: the pixel-range kernels' heal counters [kPixHealWords] (nmi_kernels.h): healed, timeouts, count-test redos
    // Split-kernel liveness (nmi_split_kernel.hip: its consumers spin, so a launch whose workgroups are not all resident
    // times out after 2 ms).  A timeout is attributed to ITS launch (epoch), that search is redone by nmi_grid_kernel, and the
    // split forms stay off for split_cooldown further small-grid launches -- 16, doubling per consecutive timeout up to
    // 4096 -- after which they are tried again; a split launch that is checked and found good re-arms the short cooldown.
    uint32_t split_timeouts = 0;           // timeouts seen so far
    uint32_t split_cooldown = 0;           // small-grid launches still to go through nmi_grid_kernel
    uint32_t split_backoff = kSplitBackoffMin;  // cooldown the next timeout starts
    uint32_t split_cooldown_epoch = 0;     // newest split epoch issued when the last cooldown was set: only launches after it re-arm the short one
    static constexpr uint32_t kSplitBackoffMin = 16, kSplitBackoffMax = 4096;
    int result_path = 1;                   // 1 mailbox spin (default), 0 hipMemcpyAsync + stream sync
    bool posted = false;                   // the most recent launch posts to the mailbox
    DeviceBuffer d_pair_rating;                   // float
    DeviceBuffer d_reduced_key;                   // unsigned long long: receive buffer of the RCCL all-reduce (never one of the ping-pong slots)
    PinnedBuffer score_mailbox;                   // unsigned long long [2], fine-grained: nmi_eval_pair's (score bits | sequence << 32)
    unsigned int pair_seq = 0;                    // nmi_eval_pair calls that posted so far
    int wait_mode = 0;                            // NMI_OPT_WAIT_MODE: 0 spin on the mailbox, 1 yield the core between polls
    // Visiting orders of the candidates (XCD-aware tiling), one per grid shape seen, so that a coarse-to-fine search
    // alternating between shapes (translation level 27 x 1, rotation level 1 x 27, ...) never waits for the stream.
    struct OrderEntry {
        int S = -1, Wn = -1;
        int grid = 0;    // workgroups of the launch the order was built for (one warp per workgroup), 0: the tiles
        DeviceBuffer d;  // int [S * Wn], or larger: an entry keeps the largest table it has held
        PinnedBuffer h;
        uint64_t last_use = 0;
    };
    static constexpr int kOrderCache = 16;
    OrderEntry orders[kOrderCache];
    uint64_t order_clock = 0;
    int xcd_tiling = 1;                   // NMI_OPT_XCD_TILING
    DeviceBuffer d_slabs;                 // nmi::SplitSlab: hand-off slabs of the split kernel, one per candidate
    DeviceBuffer d_blocks;                // counter blocks (granules) of the split kernel's pixel parts
    uint32_t split_epoch = 0;             // tag of the latest split launch
    PinnedBuffer split_error;             // uint32_t [nmi::kSplitRing], mapped: word (epoch % kSplitRing) = epoch of a launch whose hand-off timed out
    DeviceBuffer d_pix_blocks;            // hand-off blocks of nmi_pix_kernel (mid-size grids)
    // nmi_eval_pairs: pointer tables [2][pairs_cap] in pinned, mapped host memory (renders, then warps) + device scores
    PinnedBuffer pair_table;              // const uint8_t * [2 * pairs_cap]
    DeviceBuffer d_pair_scores;           // float [pairs_cap]
    int pairs_cap = 0;
    int split_pixels = -1;                // NMI_OPT_SPLIT_PIXELS: -1 automatic, 1 / 2 / 4 (with NMI_OPT_SPLIT 1: 2 ... 8)
    // Few-levels path (nmi_fewlevels_kernel.hip): which kernels score a search is decided from what the last probe of
    // the stacks found, posted by the device to *level_post = probe number << 32 | nr << 16 | nw.
    DeviceBuffer d_plan;                  // nmi::LevelPlan
    PinnedBuffer level_post;              // unsigned long long, fine-grained
    uint32_t level_seq = 0;               // probes enqueued so far
    uint32_t level_seen = 0;              // number of the probe the hint below comes from
    bool few_hint = false;                // the last probe seen found nr * nw <= fewlevels_bins
    int content_path = -1;                // NMI_OPT_CONTENT_PATH: -1 automatic (hint), 0 nmi_grid_kernel only, 1 few-levels first
    int fewlevels_bins = 4096;            // NMI_OPT_FEWLEVELS_BINS: largest nr * nw sent down the few-levels path
    DeviceBuffer d_rank_stacks;           // rank images of the search in flight: renders, then warps
    unsigned long long *dbg_stamps = nullptr;  // NMI_OPT_STAMPS
    int stamp_candidate = 0;                   // NMI_OPT_STAMP_CANDIDATE
    int split_mode = -1;                  // NMI_OPT_SPLIT: -1 automatic, 0 never, 2 / 4 / 8 row parts whenever the grid fits, 1: pixel ranges only
    DeviceBuffer d_zbuf;                  // depth|colour anchor buffers of the point-cloud renderer (padded, per view)
    DeviceBuffer d_no_red;                // float zeros: the colours of a cloud drawn without any (nmi_render_points_depth, d_red NULL)
    MeshWorkArea mesh;                     // mesh renderer (nmi_render_mesh): bins, their state, key buffer, clip queue -- for mesh_views views
    int mesh_views = 0;
    unsigned long long tile_queue_limit = 4ull << 20;  // NMI_OPT_TILE_QUEUE: usable entries per bin (capped by the bins' size)
    unsigned long long clip_queue_limit = ~0ull;       // NMI_OPT_CLIP_QUEUE
    nmi_mem::UploadRing mvp_ring, warp_ring;  // view matrices of the renderers, inverse homographies of the warp producer
    DeviceBuffer d_scratch;               // drained-counter slabs of the pipelined kernel
    int scratch_workgroups = 0;
    // Masked search (nmi_capi_masked.cpp): per-warp mask counts and term tables.  Allocated on first use, grown on demand.
    DeviceBuffer d_mask_counts;           // int32_t [warps] len_w of the latest masked search
    DeviceBuffer d_mask_tables;           // float [warps][npix + 1]
    int mask_count_n = 0;                 // warps counted by the latest masked search
    // The redo list of the masked and the covered searches' optimistic launches: one for both, as in a level or a stream (the
    // searches are serialised on the context's stream, and each leaves the list empty).
    DeviceBuffer d_mask_redo;             // int32_t: candidates to score again exactly
    DeviceBuffer d_mask_redo_state;       // uint32_t [2]: entries in the list, exact workgroups finished (zero between searches)
    // Covered search (nmi_capi_covered.cpp): per-candidate pixel counts.
    DeviceBuffer d_cover_counts;          // int32_t len[w][s] of the latest covered search, layout [Wn][S]
    int64_t cover_count_n = 0;            // candidates counted by the latest covered search
    // Deep grey frames (nmi_capi_tone.cpp): the tone map nmi_gray_frame, nmi_reduce_frame and nmi_tone_lut read at call time
    // (nmi_set_tone_map), and its histogram and table.
    nmi::ToneSetting tone;
    nmi_internal::ToneWork tone_work;
    nmi::ValidRange valid;                // nmi_set_valid_range: which raw values count in those statistics and in validity masks
    // Ranked peaks (nmi_capi_peaks.cpp): where nmi_rank_peaks' kernel writes its keys when the caller reads them back -- mapped
    // host memory, so that the blocking form is one launch and one polled word, no copy.  Allocated on first use.
    PinnedBuffer h_peaks;                 // unsigned long long [nmi::kPeaksMaxK + 1], fine-grained: the keys, then the number of the call that wrote them
    unsigned long long peaks_seq = 0;     // blocking nmi_rank_peaks calls so far
    // Refined peaks (nmi_capi_refine.cpp): the same for nmi_refine_peaks -- one posted word per record, since each record is a
    // workgroup of its own.  Allocated on first use.
    PinnedBuffer h_refine;                // fine-grained: nmi_refined_peak [nmi::kRefineMaxK], then unsigned long long [nmi::kRefineMaxK]: the number of the call that wrote record k
    unsigned long long refine_seq = 0;    // blocking nmi_refine_peaks calls so far
    nmi_mem::Event ev_start, ev_stop;
    int hist_variant = 3;
    int phase_mask = 3;
    int workgroups = 0;
    bool profiling = false;
    bool have_timing = false;
    std::string detail;
};

// nmi_texture (nmi_texture_create): mip chain of a mesh texture as per-level fp32 luma on the device.
struct nmi_texture {
    nmi_ctx *ctx = nullptr;
    DeviceBuffer d_luma;  // float
    int levels = 0;
    int w[16] = {}, h[16] = {};
    long long off[16] = {};
};

namespace nmi_internal {

// Device buffers of the mesh renderer for S views, allocated and brought to their clean state (the renderer keeps them clean).
int mesh_work_alloc(nmi_ctx *ctx, int S, MeshWorkArea *w);
int ensure_mesh_work(nmi_ctx *ctx, int S);  // the context's own, grown on demand
int ensure_mesh_pairs(nmi_ctx *ctx, MeshWorkArea *w, long long n_triangles);  // the pair list of the two-kernel binning pass
// The 9 floats the warp kernels take for one forward homography (nmi_capi_producers.cpp): NMI_ERR_INVALID_ARGUMENT for a
// non-finite or singular matrix.  Shared by nmi_warp_stack, nmi_warp_stack_masked and the level replays.
int warp_inverse_coeffs(const double *forward /*[9]*/, float *coeffs /*[9]*/);
// The sprite side for a point size (include/nmi_hip.h, nmi_render_points): NMI_ERR_INVALID_ARGUMENT for NaN, else the size
// rounded to nearest and clamped to [1, 64] in float before the conversion to int.  Shared by render_points_impl and
// nmi_level_create.
int point_sprite_size(float point_size, int *size);
int level_enqueue(nmi_level *lv, const float *h_mvps, const double *h_forward, const unsigned long long **d_key);
nmi_ctx *level_ctx(nmi_level *lv);
// ncclAllReduce(ncclMax, ncclUint64) of one 8-byte key on the context's stream, out of place (nmi_capi_rccl.cpp)
int rccl_allreduce_key(nmi_ctx *ctx, const unsigned long long *d_send, unsigned long long *d_recv, void *nccl_comm);

int hip_fail(nmi_ctx *ctx, hipError_t e, const char *what);
void build_order(int S, int Wn, int *order);
int ensure_order(nmi_ctx *ctx, int S, int Wn, int grid, const int **d_order);
// What is to be scored: the S_local x Wn block at (s_offset, w_offset) of an S_total-render grid.  A call site names what it uses.
struct SearchRequest {
    const uint8_t *render_stack = nullptr, *warp_stack = nullptr;
    int S_local = 0, s_offset = 0, S_total = 0, Wn = 0, w_offset = 0;
    float *d_ratings = nullptr;
    unsigned long long *out_key = nullptr;  // optional device word that receives the packed key
    bool post = false;                      // the caller polls the mailbox for the winner (blocking calls)
    bool post_score = false;                // ... the score mailbox (nmi_eval_pair)
    uint32_t *dbg_joint = nullptr, *dbg_h1 = nullptr, *dbg_h2 = nullptr;
    float *dbg_sums = nullptr;
    bool caller_checks_split = false;       // the caller looks for a split-kernel timeout itself (stream tickets, RCCL form)
    // nmi_eval_pairs: candidate p scores (pair_renders[p], pair_warps[p]); device views, and the caller's arrays (alignment check)
    const uint8_t *const *pair_renders = nullptr, *const *pair_warps = nullptr;
    const uint8_t *const *pair_renders_host = nullptr, *const *pair_warps_host = nullptr;
    // the block alone, in the order of the C ABI's entry points
    static SearchRequest block(const uint8_t *renders, int S_local, int s_offset, int S_total, const uint8_t *warps, int Wn, int w_offset = 0)
    {
        SearchRequest rq;
        rq.render_stack = renders;
        rq.warp_stack = warps;
        rq.S_local = S_local;
        rq.s_offset = s_offset;
        rq.S_total = S_total;
        rq.Wn = Wn;
        rq.w_offset = w_offset;
        return rq;
    }
};
// The mask side of a masked or covered search: the covered search when render_masks is set (counts receives len[w][s],
// [Wn][S_local]), else the masked one (counts: len_w [Wn], tables: the warps' term tables).  redo has room for S_local * Wn
// candidates; redo_state [2] is zero.
struct MaskSide {
    const uint8_t *warp_masks = nullptr, *render_masks = nullptr;
    int32_t *counts = nullptr;
    const float *tables = nullptr;
    int32_t *redo = nullptr;
    uint32_t *redo_state = nullptr;
};
// The grid arguments every search starts from: the request's block, the frame geometry, the key slots of this launch.
nmi::GridArgs grid_args(const nmi_ctx *ctx, const SearchRequest &rq, bool post, bool post_score);
// The scalars of the context the planner reads (nmi_search_plan.h); the caller adds those of its launch.
nmi::PlanInputs plan_inputs(const nmi_ctx *ctx, nmi::SearchForm form, int64_t total, const nmi::GridArgs &a);
double pix_owner_share(const nmi_ctx *ctx, int pix);  // the owner's share of the pixels of a pixel-range launch
// What every pixel-range launch needs beside its blocks: a hand-off epoch (a new one unless *epoch is set: a level keeps its
// own) and the context's counter of healed timeouts
int prepare_pix_handoff(nmi_ctx *ctx, uint32_t *epoch);
// The buffers the planned launch needs, grown on demand, and their pointers, the epoch and the probe's plan into a
int prepare_search(nmi_ctx *ctx, const nmi::SearchPlan &plan, nmi::GridArgs &a);
// The protocol state after an accepted launch (or an empty search: launched = false): sequence numbers, key slot, ctx->last
int commit_launch(nmi_ctx *ctx, bool post, bool post_score, const SearchLaunch &rec, bool launched, SearchLaunch *out);
// Enqueues the search (its launches, nothing else).  No synchronisation.  *launched (optional) receives what ctx->last does.
int enqueue_grid(nmi_ctx *ctx, const SearchRequest &rq, SearchLaunch *launched = nullptr);
// The masked and covered searches' kernel arguments around the grid arguments a (nmi_capi_masked.cpp)
struct MaskSearch {
    bool covered;
    nmi::MaskedGridArgs masked;
    nmi::CoveredGridArgs cover;
};
MaskSearch mask_search_args(const nmi::GridArgs &a, const MaskSide &m);
// Its launches: the pixel-range form when pix > 0 (replay, healed: as launch_pix_masked / _covered), else the grid form.
hipError_t launch_mask_search(const MaskSearch &ms, int pix, double owner_share, int workgroups, bool use_bg, bool exact,
                              const uint32_t *replay, uint32_t *healed, hipStream_t stream);
int ensure_mask_redo(nmi_ctx *ctx, int64_t total);  // the context's redo list, room for `total` candidates
// The masked / covered search's launches without its blocking tail (nmi_capi_masked.cpp): serves nmi_search_grid_masked,
// nmi_search_grid_covered and the masked / covered stream tickets.  S_local * Wn > 0; see the definition.
int enqueue_grid_mask(nmi_ctx *ctx, const SearchRequest &rq, const MaskSide &m, SearchLaunch *launched = nullptr);
int wait_word(nmi_ctx *ctx, const volatile unsigned long long *word, unsigned long long mask, unsigned long long want,
              unsigned long long *out);
int stage_floats(nmi_ctx *ctx, nmi_mem::UploadRing &ring, const float *h_src, size_t n, float **d_out);
int fetch_key(nmi_ctx *ctx, unsigned long long *key);
bool split_timed_out(nmi_ctx *ctx);                                     // ... the most recent launch
bool split_launch_failed(nmi_ctx *ctx, const SearchLaunch &launch);     // ... this launch (waits for the stream on a hit)
// what nmi_last_error_detail says after a call that was redone because of such a timeout (the call itself succeeded)
extern const char *const kSplitTimeoutNote, *const kSplitTimeoutTicketNote, *const kSplitTimeoutTicketLost;
// nmi_search_grid_block without the argument checks; caller_checks: the caller looks for a split timeout itself, so small
// grids may use the split kernel although the call only enqueues (h_key == nullptr)
int search_block(nmi_ctx *ctx, const uint8_t *render_stack, int32_t S_local, int32_t s_offset, int32_t S_total, const uint8_t *warp_stack,
                 int32_t Wn_local, int32_t w_offset, int32_t Wn_total, float *d_ratings, uint64_t *d_key, uint64_t *h_key,
                 bool caller_checks);
// What a renderer or a level draws: a coloured point cloud (attribute: red [N]), a textured mesh (uv [3T][2] + texture) or a
// vertex-coloured mesh (red [3T], no texture).
enum class MapKind { points, textured_mesh, colored_mesh };
// nmi_render_points / nmi_render_mesh / nmi_render_mesh_colored and their masked forms (nmi_capi_producers.cpp): cover = null,
// or the coverage masks.  render_mesh_impl: kind is one of the two mesh kinds, d_attr its attribute array, tex the texture
// (textured_mesh) or null (colored_mesh).
// depth (nmi_render_points_depth, nmi_render_mesh_depth): the checked shade with its depth16; the render is the depth render, a
// cloud's d_red may then be null (zeros of the context's stand in) and a mesh's d_attr is not read.
int render_points_impl(nmi_ctx *ctx, const float *d_xyz, const float *d_red, int64_t n_points, const float *h_mvps, int32_t S,
                       float point_size, uint8_t *d_render_stack, uint8_t *cover, const nmi::DepthShade *depth = nullptr);
int render_mesh_impl(nmi_ctx *ctx, MapKind kind, const float *d_xyz, const float *d_attr, int64_t n_triangles, const nmi_texture *tex,
                     const float *h_mvps, int32_t S, uint8_t *d_render_stack, uint8_t *cover, const nmi::DepthShade *depth = nullptr);
// The argument check of every depth entry point (include/nmi_hip.h, "Depth maps"), before any HIP call: NMI_OK with the kernels'
// form of the shade (depth16 null) in *out, or NMI_ERR_INVALID_ARGUMENT.
int depth_shade_check(const nmi_depth_shade *shade, nmi::DepthShade *out);
nmi::MeshShading mesh_shading(MapKind kind, const float *d_attr, const nmi_texture *tex);  // launch_render_mesh's description of a mesh kind
// The renderers' records as a context fills them: a render of the context's frame size; the mesh renderer's queue limits (NMI_OPT_*).
nmi::RenderTarget render_target(const nmi_ctx *ctx, uint8_t *out, uint8_t *cover, const nmi::DepthShade *depth);
nmi::MeshLimits mesh_limits(const nmi_ctx *ctx, int layout_views);
int check_grid_args(nmi_ctx *ctx, const uint8_t *render_stack, int S_local, int s_offset, int S_total, const uint8_t *warp_stack,
                    int Wn);

#define NMI_HIP_TRY(ctx, call)                                  \
    do {                                                        \
        hipError_t e_ = (call);                                 \
        if (e_ != hipSuccess) return nmi_internal::hip_fail((ctx), e_, #call); \
    } while (0)

// The first error of a run of HIP calls: ok(call) keeps it in ok.e and says whether this call succeeded.
struct FirstError {
    hipError_t e = hipSuccess;
    bool operator()(hipError_t r)
    {
        if (e == hipSuccess) e = r;
        return r == hipSuccess;
    }
};

struct DeviceGuard {
    int prev = -1;
    bool active = false;
    explicit DeviceGuard(int dev)
    {
        if (hipGetDevice(&prev) == hipSuccess && prev != dev) active = hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceGuard()
    {
        if (active) (void)hipSetDevice(prev);
    }
};

}  // namespace nmi_internal
