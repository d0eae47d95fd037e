// nmi_capi_pipeline.cpp -- C ABI of the composed forms: one search level as a captured HIP graph (nmi_level_*) and the
// double-buffered streaming pipeline (nmi_stream_*).  Declared in include/nmi_hip.h.
#include "nmi_covered.h"
#include "nmi_color.h"
#include "nmi_ctx.h"
#include "nmi_intake.h"
#include "nmi_mask_bits.h"
#include "nmi_masked.h"
#include "nmi_peaks.h"
#include "nmi_reduce.h"
#include "nmi_refine.h"
#include "nmi_undistort.h"

using namespace nmi_internal;

extern "C" {

// ---------------------------------------------------------------------------------------------------------
// One search level as a captured HIP graph: cloud -> S renders, frame -> Wn warps, grid search, winner to the host.
// One chain of kernel nodes and no copy nodes replays with one hipGraphLaunch (point cloud):
//   prep    reads the pinned parameter buffers, resets the key, bumps the replay parity; its other workgroups test the cloud's
//           64-point boxes -- a lane per box -- against the six planes around all views and list the survivors
//   front   a bounded number of splat workgroups over that list + the warp stack's workgroups + the clear of the NEXT replay's
//           anchor buffer
//   resolve sprites from anchors
//   search  whose last workgroup stores the winner into pinned host memory.
// (Textured or vertex-coloured mesh: prep -> binning + warp workgroups -> clip -> tiles -> search.  Where the warp cannot ride along -- frame rows
// not 16-byte aligned -- it runs on a forked branch.)  Only the pinned parameter buffers change between replays; the caller
// polls the winner word.
// ---------------------------------------------------------------------------------------------------------
}  // extern "C"

// What a level's setters change.  A refused or failed call leaves the whole value as it was.
struct LevelSettings {
    bool masked = false, covered = false;
    const uint8_t *d_frame_mask = nullptr;      // the caller's, read in place on every replay
    FrameIntake intake;
    bool depth = false;                         // the renders are depth renders (nmi_level_set_depth_shade), shaded by ...
    nmi::DepthShade shade{};                    // ... this (checked; its depth16 null: a level keeps no raw depths)
    nmi::PeaksArgs peaks{};                     // nmi_level_set_peaks: K, the table's shape and the radii (checked); K = 0: off
    bool refine = false;                        // nmi_level_set_refine: the peaks are refined too (only with peaks.K > 0)
};

struct nmi_level {
    nmi_ctx *ctx = nullptr;
    int S = 0, Wn = 0, size = 1;                // this rank's block: S views x Wn warps ...
    int s_offset = 0, S_total = 0, w_offset = 0, Wn_total = 0;  // ... of an S_total x Wn_total level (block == level on one rank)
    DeviceBuffer d_renders, d_warps;            // uint8_t [S][H][W], [Wn][H][W]
    DeviceBuffer d_zbuf;                        // uint32_t, point cloud: anchor buffer
    DeviceBuffer d_packed;                      // point cloud: the level's own packed copy of the cloud (16-byte records + wavefront boxes)
    MeshWorkArea mesh;                          // either mesh kind: the renderer's work area (kept clean by the renderer itself)
    MapKind kind = MapKind::points;             // what the level draws; d_attr below is red [N], uv [3T][2] or red [3T] accordingly
    bool no_attr = false;                       // created without attributes (nmi_level_create_depth): it has depth renders only.  A cloud's
    DeviceBuffer d_no_red;                      // "colours" are then these zeros, float [N]; a mesh's d_attr is null (kind colored_mesh)
    bool fused_points = false;                  // point cloud, one chain of kernels, double-buffered anchors
    DeviceBuffer d_kept, d_kept_count;          // uint32_t: ... and the wavefronts in reach of a view, listed by the prep kernel per replay
    uint32_t replay = 0;                        // parity of the counters the prep kernel counts under
    DeviceBuffer d_mvps, d_coeffs;              // float
    PinnedBuffer h_mvps, h_coeffs;              // float, mapped: the prep kernel reads this replay's parameters from them
    DeviceBuffer d_order;                       // int
    DeviceBuffer d_ratings;                     // float [Wn][S] rating table of the latest replay
    DeviceBuffer d_key;                         // unsigned long long
    PinnedBuffer h_key;                         // unsigned long long, mapped: the search kernel posts the winner
    DeviceBuffer d_done;                        // unsigned int
    DeviceBuffer d_epoch;                       // uint32_t: replays so far, bumped by the prep kernel: parity of the double-buffered anchors (fused
                                                // point-cloud form), tag of the search kernel's hand-offs (nmi_pix_kernel)
    DeviceBuffer d_pix_blocks;                  // nmi_pix_kernel's hand-off blocks when the level's grid is a mid-size one
    int pix = 0;                                // pixel ranges per candidate of the captured search (0: nmi_grid_kernel)
    nmi_mem::Stream side;                       // forked capture branch (warp)
    nmi_mem::Event ev_fork, ev_join;
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    // What the graph is captured from (level_capture), kept so that level_apply can capture it again.
    const float *d_xyz = nullptr, *d_attr = nullptr;
    int64_t n_points = 0;
    const nmi_texture *tex = nullptr;
    const uint8_t *d_frame = nullptr;
    nmi::GridArgs args{};                       // the search's arguments (unmasked form)
    int workgroups = 0;
    // What the setters change, as one value (level_apply): masks (nmi_level_set_masks) or coverage (nmi_level_set_coverage, never
    // both at once), their frame mask, and the frame's way in (nmi_level_set_distortion, _set_frame_format, _set_frame_reduction,
    // _set_tone_map, _set_valid_range), and what the renders show (nmi_level_set_depth_shade).
    LevelSettings set;
    // The buffers that go with the settings: level_buffers says which of them a setting needs, level_apply allocates and frees.
    // Masked: the warps' masks and counts of the latest replay, the counts of the replay before (tables are rebuilt only for the
    // warps whose count changed), the per-warp term tables, the redo list of the masked grid kernel.
    DeviceBuffer d_masks;                       // uint8_t [Wn][H][W]
    DeviceBuffer d_counts;                      // int32_t [3][Wn]: counts, previous counts, changed flags
    DeviceBuffer d_tables;                      // float [Wn][npix + 1]
    DeviceBuffer d_redo;                        // int32_t [S * Wn]
    DeviceBuffer d_redo_state;                  // uint32_t [2], zero between replays
    // Covered: the renders' coverage masks and len[w][s] of the latest replay; the warps' masks and the redo list are the masked
    // level's fields above.
    DeviceBuffer d_rmasks;                      // uint8_t [S][H][W], render layout
    DeviceBuffer d_cover_counts;                // int32_t [Wn][S]
    // Distorted, coloured or reduced: d_frame (and d_frame_mask) are the camera's frame; every replay brings it into d_ud, the
    // level's own grey frame (and, distorted and masked or covered, its mask into d_ud_mask), which the warps and their masks read
    // instead.  Reduced (or a Bayer mosaic, or a deep frame) and distorted: brought to grey in d_small, which the undistortion
    // node reads in d_frame's place.
    DeviceBuffer d_ud, d_ud_mask, d_small;      // uint8_t [H][W] each
    // A deep frame under a valid range, masked or covered: the validity mask its conversion node writes (ANDed with d_frame_mask,
    // which stays the caller's, read only): the frame mask of the warp masks, or, distorted, the undistortion node's raw mask.
    DeviceBuffer d_valid;                       // uint8_t [H][W]
    // Ranked peaks (nmi_level_set_peaks): the keys of the latest replay, written by the node after the search.
    DeviceBuffer d_peaks;                       // unsigned long long [nmi::kPeaksMaxK]
    // Refined peaks (nmi_level_set_refine): the records of the latest replay, written by the node after the peaks node.
    DeviceBuffer d_refined;                     // nmi_refined_peak [nmi::kRefineMaxK]
    // A deep frame (GRAY16): its tone map's histogram and table (nmi_tone.h), prepared by level_apply before the capture.
    ToneWork tone_work;
};

extern "C" {

int nmi_level_destroy(nmi_level *lv)
{
    if (!lv) return NMI_OK;
    DeviceGuard guard(lv->ctx->device);
    (void)hipStreamSynchronize(lv->ctx->stream);
    if (lv->exec) (void)hipGraphExecDestroy(lv->exec);
    if (lv->graph) (void)hipGraphDestroy(lv->graph);
    delete lv;
    return NMI_OK;
}

}  // extern "C"

// Which of the level's setting buffers (struct nmi_level) a setting needs.  This is the one place that says so: level_apply
// allocates and frees by it, level_capture reads by it.
struct LevelNeeds {
    bool mode;     // masked or covered: d_masks, d_redo, d_redo_state
    bool masks;    // masked: d_counts, d_tables
    bool cover;    // covered: d_rmasks, d_cover_counts
    bool ud;       // the level's own grey frame
    bool ud_mask;  // ... and its mask: undistorted, for the warps' masks
    bool small;    // the reduced (or demosaiced, or tone-mapped) grey frame the undistortion node reads
    bool valid;    // the validity mask of a deep frame under a valid range, for the warps' masks: d_valid
    bool peaks;    // ranked peaks: d_peaks
    bool refine;   // refined peaks: d_refined
};

static LevelNeeds level_needs(const LevelSettings &s)
{
    const bool mode = s.masked || s.covered;
    return {mode, s.masked, s.covered, s.intake.own_frame(), s.intake.distorted && mode, s.intake.two_nodes(), s.intake.validity() && mode,
            s.peaks.K > 0, s.refine};
}

struct LevelBuffer {
    DeviceBuffer *slot;
    size_t bytes, zeroed;  // its size, and how much of it starts as zero
    bool needed;
};

static std::vector<LevelBuffer> level_buffers(nmi_level *lv, const LevelSettings &s)
{
    const LevelNeeds n = level_needs(s);
    const size_t npix = (size_t)lv->ctx->npix, S = (size_t)lv->S, Wn = (size_t)lv->Wn, cells = S * Wn * sizeof(int32_t);
    return {{&lv->d_masks, npix * Wn, npix * Wn, n.mode},
            {&lv->d_redo, cells, 0, n.mode},
            {&lv->d_redo_state, 2 * sizeof(uint32_t), 2 * sizeof(uint32_t), n.mode},
            {&lv->d_counts, 3 * Wn * sizeof(int32_t), Wn * sizeof(int32_t), n.masks},
            {&lv->d_tables, Wn * (npix + 1) * sizeof(float), 0, n.masks},
            {&lv->d_rmasks, npix * S, npix * S, n.cover},
            {&lv->d_cover_counts, cells, cells, n.cover},
            {&lv->d_ud, npix, 0, n.ud},
            {&lv->d_ud_mask, npix, 0, n.ud_mask},
            {&lv->d_small, npix, 0, n.small},
            {&lv->d_valid, npix, 0, n.valid},
            {&lv->d_peaks, nmi::kPeaksMaxK * sizeof(unsigned long long), nmi::kPeaksMaxK * sizeof(unsigned long long), n.peaks},
            {&lv->d_refined, nmi::kRefineMaxK * sizeof(nmi_refined_peak), nmi::kRefineMaxK * sizeof(nmi_refined_peak), n.refine}};
}

// Captures the level's graph for lv->set and instantiates it, replacing the previous one only on success.  The caller has waited
// for the stream and holds the buffers lv->set needs (level_apply; a level as created needs none).
static int level_capture(nmi_level *lv)
{
    nmi_ctx *ctx = lv->ctx;
    const nmi_params &p = ctx->params;
    const int S = lv->S, Wn = lv->Wn;
    const int64_t total = (int64_t)S * Wn;
    const nmi_texture *tex = lv->tex;
    const bool mesh = lv->kind != MapKind::points;
    const float *d_xyz = lv->d_xyz, *d_attr = lv->d_attr, *d_red = lv->d_attr;
    const int64_t n_points = lv->n_points;
    float *hd_mvps = lv->h_mvps.device<float>(), *hd_coeffs = lv->h_coeffs.device<float>();
    // typed views of the level's buffers (null where the settings need none: level_buffers)
    uint8_t *d_renders = lv->d_renders.as<uint8_t>(), *d_warps = lv->d_warps.as<uint8_t>(), *d_masks = lv->d_masks.as<uint8_t>();
    uint8_t *d_rmasks = lv->d_rmasks.as<uint8_t>(), *d_ud = lv->d_ud.as<uint8_t>(), *d_small = lv->d_small.as<uint8_t>();
    uint32_t *d_zbuf = lv->d_zbuf.as<uint32_t>(), *d_epoch = lv->d_epoch.as<uint32_t>(), *d_kept = lv->d_kept.as<uint32_t>();
    uint32_t *d_kept_count = lv->d_kept_count.as<uint32_t>(), *d_redo_state = lv->d_redo_state.as<uint32_t>();
    float *d_mvps = lv->d_mvps.as<float>(), *d_coeffs = lv->d_coeffs.as<float>(), *d_tables = lv->d_tables.as<float>();
    int32_t *d_counts = lv->d_counts.as<int32_t>(), *d_cover_counts = lv->d_cover_counts.as<int32_t>(), *d_redo = lv->d_redo.as<int32_t>();
    void *d_packed = lv->d_packed.as<>();
    FirstError ok;
    // Distorted or coloured: the chain reads the level's own grey (undistorted) frame (16-byte aligned: the fused front kernels
    // stay eligible) and, distorted and masked or covered, its mask.  A frame mask is dense [H][W] in every format.
    const LevelSettings &set = lv->set;
    const FrameIntake &in = set.intake;
    const bool masked = set.masked, covered = set.covered;
    uint8_t *ud_mask = level_needs(set).ud_mask ? lv->d_ud_mask.as<uint8_t>() : nullptr;
    uint8_t *valid = level_needs(set).valid ? lv->d_valid.as<uint8_t>() : nullptr;  // the conversion's validity mask goes here
    const uint8_t *d_frame = in.own_frame() ? d_ud : lv->d_frame;
    const uint8_t *d_frame_mask = in.distorted ? ud_mask : valid ? valid : set.d_frame_mask;
    nmi::GridArgs a = lv->args;
    // Mid-size grids (the live strategy's collapsed levels, a rank's block of a sharded level): P workgroups per candidate
    // (nmi_pix_kernel.hip, nmi_masked_pix_kernel.hip, nmi_covered_pix_kernel.hip).  Its hand-off tag = the epoch frozen into the graph + the replay count the
    // prep kernel keeps; the level keeps one epoch for all its captures (the replay count only grows, so tags never repeat).
    const nmi::SearchPlan plan = nmi::plan_search(plan_inputs(ctx, nmi::SearchForm::level, total, a));
    lv->pix = plan.pix;
    if (lv->pix) {
        const size_t bytes = nmi::pix_block_bytes((int)total, lv->pix);
        // (no wait of its own: level_apply has waited; cleared at once, not on the stream)
        if (bytes > lv->d_pix_blocks.size() && ok(lv->d_pix_blocks.grow(bytes)) && !ok(hipMemset(lv->d_pix_blocks.as<>(), 0, bytes)))
            (void)lv->d_pix_blocks.reset();
        if (ok.e == hipSuccess && prepare_pix_handoff(ctx, &lv->args.epoch) != NMI_OK) ok.e = hipErrorOutOfMemory;
        if (ok.e == hipSuccess) ok(hipStreamSynchronize(ctx->stream));
        a.epoch = lv->args.epoch;
        a.blocks = lv->d_pix_blocks.as<unsigned long long>();
        a.order = nullptr;
    }
    const int workgroups = lv->workgroups;
    nmi::GridArgs ma = a;
    ma.phase_mask = plan.phase_mask;  // (bit 9: the pixel-range kernel's hand-off test hook)
    const MaskSearch ms = mask_search_args(ma, MaskSide{d_masks, covered ? d_rmasks : nullptr, covered ? d_cover_counts : d_counts,
                                                        d_tables, d_redo, d_redo_state});
    uint8_t *cover = covered ? d_rmasks : nullptr;  // the renderers' coverage masks
    const nmi::DepthShade *depth = set.depth ? &set.shade : nullptr;  // the renderers' shade: the map's colour, or its depth
    int32_t *d_prev = d_counts + Wn, *d_changed = d_counts + 2 * Wn;
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    hipStream_t st = ctx->stream;
    if (ok.e == hipSuccess && ok(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal))) {
        nmi::FusedCloud cloud{};  // a fused point-cloud level's packed cloud and kept list; else empty
        if (lv->fused_points) {
            cloud.packed = d_packed, cloud.npoints = n_points;
            cloud.h_bound = hd_mvps + (size_t)S * 16;
            cloud.kept = d_kept, cloud.kept_count = d_kept_count;
        }
        nmi::LevelPrep prep{};
        prep.h_mvps = hd_mvps, prep.d_mvps = d_mvps, prep.n_mvps = S * 16 + nmi::kLevelMvpExtra;
        prep.h_coeffs = hd_coeffs, prep.d_coeffs = d_coeffs, prep.n_coeffs = Wn * 9;
        prep.key = lv->d_key.as<unsigned long long>();
        // (mesh: nothing to clear -- the renderer leaves its work area clean)
        prep.zbuf = d_zbuf, prep.nz = (mesh || lv->fused_points) ? 0 : nmi::render_zbuf_words(S, p.width, p.height, lv->size);
        prep.epoch = d_epoch;
        prep.cloud = cloud;
        ok(nmi::launch_level_prep(prep, st));
        ok(launch_intake(in, lv->tone_work, lv->d_frame, in.frame_pitch, set.d_frame_mask, d_small, d_ud, ud_mask, valid, p.width, p.height,
                         st));
        // One chain of kernels when the warp blocks can ride along with the render's first kernel (the usual case: frame rows
        // 16-byte aligned); otherwise the warp kernel runs on a forked branch beside the render.
        const bool fused = mesh ? (nmi::level_front_eligible(d_frame, d_warps, p.width, S) && n_points > 0) : lv->fused_points;
        // Masked: the masks, their counts and the changed warps' tables on that branch too (they need the inverse maps only),
        // beside the render.  Covered: the masks alone (no counts, no tables: len[w][s] is counted by the search).
        if (!fused || masked || covered) {
            ok(hipEventRecord(lv->ev_fork, st));
            ok(hipStreamWaitEvent(lv->side, lv->ev_fork, 0));
            if (!fused) ok(nmi::launch_warp(d_frame, d_coeffs, d_warps, p.width, p.height, Wn, lv->side));
            if (masked) {
                ok(nmi::launch_warp_masks(d_frame_mask, d_coeffs, d_masks, p.width, p.height, Wn, lv->side));
                ok(nmi::launch_level_mask_counts(d_masks, Wn, ctx->npix, d_counts, d_prev, d_changed, lv->side));
                ok(nmi::launch_level_mask_tables(d_counts, d_changed, Wn, ctx->npix, d_tables, lv->side));
            }
            if (covered) ok(nmi::launch_warp_masks(d_frame_mask, d_coeffs, d_masks, p.width, p.height, Wn, lv->side));
            ok(hipEventRecord(lv->ev_join, lv->side));
        }
        // The render, by whichever of the three renderers the level uses: the same target, views and (fused) ride-along warp.
        const nmi::RenderTarget target = render_target(ctx, d_renders, cover, depth);
        const nmi::RenderViews views{d_mvps, S};
        nmi::RideAlongWarp warp{};
        if (fused) warp.frame = d_frame, warp.coeffs = d_coeffs, warp.out = d_warps, warp.Wn = Wn;
        if (mesh)
            ok(nmi::launch_render_mesh(d_xyz, mesh_shading(lv->kind, d_attr, tex), n_points, views, lv->mesh.view, mesh_limits(ctx, S), target, st, warp));
        else if (fused)
            ok(nmi::launch_level_front_points(cloud, views, d_zbuf, d_epoch, lv->size, ctx->compute_units, target, warp, st));
        else
            ok(nmi::launch_render_points(d_xyz, d_red, n_points, views, d_zbuf, lv->size, target, st, /*clear_first=*/false));
        if (!fused || masked || covered) ok(hipStreamWaitEvent(st, lv->ev_join, 0));
        if (masked || covered)
            ok(launch_mask_search(ms, lv->pix, lv->pix ? pix_owner_share(ctx, lv->pix) : 0.0, workgroups, true, false, d_epoch,
                                  ctx->d_pix_timeouts.as<uint32_t>(), st));
        else if (lv->pix)
            ok(nmi::launch_pix(a, lv->pix, pix_owner_share(ctx, lv->pix), true, d_epoch, ctx->d_pix_timeouts.as<uint32_t>(), st));
        else
            ok(nmi::launch_grid(a, workgroups, true, st));
        // Ranked peaks: one more node on the main chain, after the search (whichever of its kernels) has filled the table.
        if (set.peaks.K > 0) {
            nmi::PeaksArgs pk = set.peaks;
            pk.ratings = a.ratings;
            pk.out = lv->d_peaks.as<unsigned long long>();
            ok(nmi::launch_peaks(pk, st));
            // Refined peaks: one more node behind it, reading the keys it wrote and the same table.
            if (set.refine) {
                nmi::RefineArgs rf;
                rf.ratings = a.ratings;
                for (int i = 0; i < 6; ++i) rf.num[i] = pk.num[i];
                rf.cells = (uint32_t)pk.cells;
                rf.K = pk.K;
                rf.keys = pk.out;
                rf.out = lv->d_refined.as<nmi_refined_peak>();
                ok(nmi::launch_refine(rf, st));
            }
        }
        hipError_t ec = hipStreamEndCapture(st, &graph);
        ok(ec);
    }
    if (ok.e == hipSuccess) ok(hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));
    if (ok.e != hipSuccess) {
        if (exec) (void)hipGraphExecDestroy(exec);
        if (graph) (void)hipGraphDestroy(graph);
        return hip_fail(ctx, ok.e, "nmi_level (graph capture)");
    }
    if (lv->exec) (void)hipGraphExecDestroy(lv->exec);
    if (lv->graph) (void)hipGraphDestroy(lv->graph);
    lv->graph = graph;
    lv->exec = exec;
    return NMI_OK;
}

// Every setter's transaction: the level takes the settings `next` and captures its graph again, or stays exactly as it was.
// all_tables (nmi_level_set_masks, enabling): the new graph's first replay builds every warp's term table.
static int level_apply(nmi_level *lv, const LevelSettings &next, const char *what, bool all_tables = false)
{
    nmi_ctx *ctx = lv->ctx;
    ctx->detail.clear();
    if (lv->S == 0 || lv->Wn == 0) {  // empty block: no graph; it only takes part in the exchange
        lv->set = next;
        return NMI_OK;
    }
    DeviceGuard guard(ctx->device);
    NMI_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // a replay in flight still reads the buffers and the graph
    FirstError ok;
    std::vector<DeviceBuffer *> fresh;  // allocated by this call
    for (const LevelBuffer &b : level_buffers(lv, next)) {
        if (!b.needed || *b.slot || ok.e != hipSuccess) continue;
        if (ok(b.slot->alloc(b.bytes))) fresh.push_back(b.slot);
        if (ok.e == hipSuccess && b.zeroed) ok(hipMemset(b.slot->as<>(), 0, b.zeroed));
    }
    // every warp "changed": the first replay builds all the tables (the previous counts may be another frame mask's)
    if (ok.e == hipSuccess && all_tables) ok(hipMemset(lv->d_counts.as<int32_t>() + lv->Wn, 0xFF, (size_t)lv->Wn * sizeof(int32_t)));
    // a deep frame's tone buffers, and the table of a fixed mode (outside the capture: the graph only reads it)
    // (and the container of a deep source that unpacks; it only grows, and a grown one is a new address)
    const nmi_params &p = ctx->params;
    const void *container_was = lv->tone_work.container.as<>();
    if (ok.e == hipSuccess && next.intake.deep())
        ok(tone_prepare(&lv->tone_work, next.intake.tone, ctx->stream, next.intake.container(p.width, p.height)));
    int rc = ok.e == hipSuccess ? NMI_OK : hip_fail(ctx, ok.e, what);
    const LevelSettings was = lv->set;
    if (rc == NMI_OK) {
        lv->set = next;
        rc = level_capture(lv);
    }
    if (rc != NMI_OK) {
        lv->set = was;
        for (DeviceBuffer *slot : fresh) (void)slot->reset();
        if (was.intake.deep()) {  // the old graph's table again; its container moved: the old settings captured again
            (void)tone_prepare(&lv->tone_work, was.intake.tone, ctx->stream, was.intake.container(p.width, p.height));
            if (was.intake.container(p.width, p.height) && lv->tone_work.container.as<>() != container_was) (void)level_capture(lv);
        }
        return rc;
    }
    for (const LevelBuffer &b : level_buffers(lv, lv->set))  // no graph reads these any more
        if (!b.needed) (void)b.slot->reset();
    if (!lv->set.intake.deep()) lv->tone_work = ToneWork{};
    return NMI_OK;
}

// Common part of nmi_level_create (kind points: d_attr = red), nmi_level_create_mesh (textured_mesh: d_attr = uv, tex, n =
// triangles) and nmi_level_create_mesh_colored (colored_mesh: d_attr = red per corner, no texture, n = triangles).
// depth (nmi_level_create_depth): a level without attributes -- d_attr is null, kind is points or colored_mesh -- that starts with
// this shade and can never be without one.
struct LevelBlock {
    int32_t S, s_offset, S_total, Wn, w_offset, Wn_total;
};

static int level_create(nmi_ctx *ctx, MapKind kind, const float *d_xyz, const float *d_attr, int64_t n_points, const nmi_texture *tex,
                        const uint8_t *d_frame, const LevelBlock &blk, float point_size, nmi_level **out, const nmi::DepthShade *depth = nullptr)
{
    const bool mesh = kind != MapKind::points;
    const float *d_red = d_attr;
    const int32_t S = blk.S, Wn = blk.Wn;
    if (!ctx || !out || !d_frame || S < 0 || Wn < 0 || n_points < 0 || (n_points > 0 && (!d_xyz || (!d_attr && !depth))))
        return NMI_ERR_INVALID_ARGUMENT;
    if (blk.S_total <= 0 || blk.Wn_total <= 0 || blk.s_offset < 0 || blk.w_offset < 0 || blk.s_offset + S > blk.S_total ||
        blk.w_offset + Wn > blk.Wn_total)
        return NMI_ERR_INVALID_ARGUMENT;
    if ((int64_t)blk.S_total * blk.Wn_total >= 0x7FFFFFFFll) return NMI_ERR_UNSUPPORTED;  // index lives in 32 bits of the key
    if (kind == MapKind::textured_mesh ? (!tex || tex->ctx != ctx) : tex != nullptr) return NMI_ERR_INVALID_ARGUMENT;
    int size = 1;  // (a mesh level has no point size)
    if (!mesh && point_sprite_size(point_size, &size) != NMI_OK) return NMI_ERR_INVALID_ARGUMENT;
    if (!ctx->params.use_bg) return NMI_ERR_UNSUPPORTED;
    *out = nullptr;
    ctx->detail.clear();
    DeviceGuard guard(ctx->device);
    nmi_level *lv = new (std::nothrow) nmi_level;
    if (!lv) return NMI_ERR_INVALID_ARGUMENT;
    lv->ctx = ctx;
    lv->kind = kind;
    if (depth) lv->no_attr = true, lv->set.depth = true, lv->set.shade = *depth;
    lv->S = S;
    lv->Wn = Wn;
    lv->s_offset = blk.s_offset;
    lv->S_total = blk.S_total;
    lv->w_offset = blk.w_offset;
    lv->Wn_total = blk.Wn_total;
    if (S == 0 || Wn == 0) {
        // An empty block (more ranks than cells on the sharded axis): nothing to render, warp or score.  The rank still owns
        // a key word -- "no candidate" -- for the level's collective (nmi_level_run_rccl).
        hipError_t e0 = lv->d_key.alloc(sizeof(unsigned long long));
        if (e0 == hipSuccess) e0 = hipMemset(lv->d_key.as<>(), 0, sizeof(unsigned long long));
        if (e0 != hipSuccess) {
            const int rc = hip_fail(ctx, e0, "nmi_level_create (empty block)");
            nmi_level_destroy(lv);
            return rc;
        }
        *out = lv;
        return NMI_OK;
    }
    lv->size = size;
    const nmi_params &p = ctx->params;
    const size_t npix = (size_t)ctx->npix;
    const int64_t total = (int64_t)S * Wn;
    FirstError ok;
    ok(lv->d_renders.alloc(npix * S));
    ok(lv->d_warps.alloc(npix * Wn));
    if (mesh) {
        if (mesh_work_alloc(ctx, S, &lv->mesh) != NMI_OK) ok.e = hipErrorOutOfMemory;
        if (ok.e == hipSuccess && ensure_mesh_pairs(ctx, &lv->mesh, n_points) != NMI_OK) ok.e = hipErrorOutOfMemory;
        ok(lv->d_epoch.alloc(sizeof(uint32_t)));
        if (ok.e == hipSuccess) ok(hipMemsetAsync(lv->d_epoch.as<>(), 0, sizeof(uint32_t), ctx->stream));
    } else {
        // Anchors: two buffers when the level runs as one chain of kernels (the front kernel of replay k clears the buffer of
        // replay k + 1); the classic form keeps one and clears it in its prep node.
        lv->fused_points = nmi::level_front_eligible(d_frame, nullptr, p.width, S) && n_points > 0 && nmi::level_points_double_buffered(p.width, lv->size);
        const size_t words = lv->fused_points ? 2 * nmi::level_zbuf_pair_words(S, p.width, p.height, lv->size)
                                              : nmi::render_zbuf_words(S, p.width, p.height, lv->size);
        ok(lv->d_zbuf.alloc(words * sizeof(uint32_t)));
        ok(lv->d_epoch.alloc(sizeof(uint32_t)));
        ok(lv->d_packed.alloc(nmi::cloud_pack_bytes(n_points, nullptr) + 16));
        if (depth && n_points > 0) {  // a cloud without colours: zeros stand in (the colour only breaks ties between equal depths)
            ok(lv->d_no_red.alloc((size_t)n_points * sizeof(float)));
            if (ok.e == hipSuccess) ok(hipMemsetAsync(lv->d_no_red.as<>(), 0, (size_t)n_points * sizeof(float), ctx->stream));
            d_attr = d_red = lv->d_no_red.as<float>();
        }
        if (ok.e == hipSuccess) ok(hipMemsetAsync(lv->d_zbuf.as<>(), 0xFF, words * sizeof(uint32_t), ctx->stream));
        if (ok.e == hipSuccess) ok(hipMemsetAsync(lv->d_epoch.as<>(), 0, sizeof(uint32_t), ctx->stream));
        if (ok.e == hipSuccess) ok(nmi::launch_cloud_pack(d_xyz, d_red, n_points, lv->d_packed.as<>(), ctx->stream));
        if (lv->fused_points) {
            ok(lv->d_kept.alloc((size_t)(2 * ((n_points + 63) / 64) + 1) * sizeof(uint32_t)));   // (twice the most one replay lists)
            ok(lv->d_kept_count.alloc(2 * sizeof(uint32_t)));
            if (ok.e == hipSuccess) ok(hipMemsetAsync(lv->d_kept_count.as<>(), 0, 2 * sizeof(uint32_t), ctx->stream));
        }
    }
    const size_t mvp_bytes = ((size_t)S * 16 + nmi::kLevelMvpExtra) * sizeof(float), coeff_bytes = (size_t)Wn * 9 * sizeof(float);
    ok(lv->d_mvps.alloc(mvp_bytes));
    ok(lv->d_coeffs.alloc(coeff_bytes));
    ok(lv->d_order.alloc((size_t)total * sizeof(int)));
    ok(lv->d_ratings.alloc((size_t)total * sizeof(float)));
    ok(lv->d_key.alloc(sizeof(unsigned long long)));
    ok(lv->d_done.alloc(sizeof(unsigned int)));
    // pinned, device-mapped, fine-grained: the prep kernel reads the parameters and the search kernel posts the winner
    ok(lv->h_mvps.alloc(mvp_bytes, nmi_mem::kPosted));
    ok(lv->h_coeffs.alloc(coeff_bytes, nmi_mem::kPosted));
    ok(lv->h_key.alloc(sizeof(unsigned long long), nmi_mem::kPosted));
    ok(lv->side.create(hipStreamNonBlocking));
    ok(lv->ev_fork.create(hipEventDisableTiming));
    ok(lv->ev_join.create(hipEventDisableTiming));
    int *order = ok.e == hipSuccess ? new (std::nothrow) int[(size_t)total] : nullptr;
    if (ok.e != hipSuccess || !order) {
        const int rc = ok.e != hipSuccess ? hip_fail(ctx, ok.e, "nmi_level_create") : NMI_ERR_INVALID_ARGUMENT;
        nmi_level_destroy(lv);
        return rc;
    }
    build_order(S, Wn, order);
    ok(hipMemcpy(lv->d_order.as<>(), order, (size_t)total * sizeof(int), hipMemcpyHostToDevice));
    delete[] order;
    ok(hipMemset(lv->d_done.as<>(), 0, sizeof(unsigned int)));
    memset(lv->h_mvps.as<>(), 0, mvp_bytes);
    memset(lv->h_coeffs.as<>(), 0, coeff_bytes);
    ok(hipDeviceSynchronize());

    nmi::GridArgs a{};
    a.render_stack = lv->d_renders.as<uint8_t>();
    a.warp_stack = lv->d_warps.as<uint8_t>();
    a.S_local = S;
    a.Wn = Wn;
    a.s_offset = blk.s_offset;  // global indices in the key (commit_score): the winner of a block is a cell of the whole level
    a.S_total = blk.S_total;
    a.w_offset = blk.w_offset;
    nmi::set_geometry(a, p.width, p.height, a.render_stack, a.warp_stack, p.render_bottom_up != 0);
    a.shift = ctx->shift;
    a.mode = p.mode;
    a.table = ctx->table.as<float>();
    a.order = lv->d_order.as<int>();
    a.ratings = lv->d_ratings.as<float>();  // 4 bytes per candidate: kept so that a level can be checked against an oracle (nmi_level_copy_outputs)
    a.key = lv->d_key.as<unsigned long long>();  // reset by the prep node before every replay (the ping-pong of plain launches needs
    a.reset_key = nullptr;    // alternating arguments, which a replayed graph does not have)
    a.done = lv->d_done.as<unsigned int>();
    a.out_key = lv->h_key.device<unsigned long long>();
    a.hist_variant = 3;
    a.phase_mask = 3;
    // the graph (level_capture) is made from these; level_apply captures it again from them
    lv->d_xyz = d_xyz;
    lv->d_attr = d_attr;
    lv->n_points = n_points;
    lv->tex = tex;
    lv->d_frame = d_frame;
    lv->args = a;
    lv->workgroups = nmi::grid_workgroups(total, ctx->workgroups, ctx->compute_units);
    if (ok.e == hipSuccess) {
        const int rc = level_capture(lv);
        if (rc != NMI_OK) {
            nmi_level_destroy(lv);
            return rc;
        }
    }
    if (ok.e != hipSuccess) {
        const int rc = hip_fail(ctx, ok.e, "nmi_level_create");
        nmi_level_destroy(lv);
        return rc;
    }
    *out = lv;
    return NMI_OK;
}

extern "C" {

int nmi_level_create(nmi_ctx *ctx, const float *d_xyz, const float *d_red, int64_t n_points, const uint8_t *d_frame, int32_t S,
                     int32_t Wn, float point_size, nmi_level **out)
{
    if (S <= 0 || Wn <= 0) return NMI_ERR_INVALID_ARGUMENT;
    return level_create(ctx, MapKind::points, d_xyz, d_red, n_points, nullptr, d_frame, LevelBlock{S, 0, S, Wn, 0, Wn}, point_size, out);
}

int nmi_level_create_mesh(nmi_ctx *ctx, const float *d_xyz, const float *d_uv, int64_t n_triangles, const nmi_texture *tex,
                          const uint8_t *d_frame, int32_t S, int32_t Wn, nmi_level **out)
{
    if (!tex || S <= 0 || Wn <= 0) return NMI_ERR_INVALID_ARGUMENT;
    return level_create(ctx, MapKind::textured_mesh, d_xyz, d_uv, n_triangles, tex, d_frame, LevelBlock{S, 0, S, Wn, 0, Wn}, 1.0f, out);
}

int nmi_level_create_mesh_colored(nmi_ctx *ctx, const float *d_xyz, const float *d_red, int64_t n_triangles, const uint8_t *d_frame, int32_t S,
                                  int32_t Wn, nmi_level **out)
{
    if (S <= 0 || Wn <= 0) return NMI_ERR_INVALID_ARGUMENT;
    return level_create(ctx, MapKind::colored_mesh, d_xyz, d_red, n_triangles, nullptr, d_frame, LevelBlock{S, 0, S, Wn, 0, Wn}, 1.0f, out);
}

// Depth levels: a level of a map without attributes, and the shade of any level.
int nmi_level_create_depth_block(nmi_ctx *ctx, int32_t map_kind, const float *d_xyz, int64_t n, const uint8_t *d_frame, int32_t S_local,
                                 int32_t s_offset, int32_t S_total, int32_t Wn_local, int32_t w_offset, int32_t Wn_total, float point_size,
                                 const nmi_depth_shade *shade, nmi_level **out)
{
    nmi::DepthShade sh;
    if ((map_kind != NMI_MAP_POINTS && map_kind != NMI_MAP_MESH) || depth_shade_check(shade, &sh) != NMI_OK) return NMI_ERR_INVALID_ARGUMENT;
    const bool mesh = map_kind == NMI_MAP_MESH;
    return level_create(ctx, mesh ? MapKind::colored_mesh : MapKind::points, d_xyz, nullptr, n, nullptr, d_frame,
                        LevelBlock{S_local, s_offset, S_total, Wn_local, w_offset, Wn_total}, mesh ? 1.0f : point_size, out, &sh);
}

int nmi_level_create_depth(nmi_ctx *ctx, int32_t map_kind, const float *d_xyz, int64_t n, const uint8_t *d_frame, int32_t S, int32_t Wn,
                           float point_size, const nmi_depth_shade *shade, nmi_level **out)
{
    if (S <= 0 || Wn <= 0) return NMI_ERR_INVALID_ARGUMENT;
    return nmi_level_create_depth_block(ctx, map_kind, d_xyz, n, d_frame, S, 0, S, Wn, 0, Wn, point_size, shade, out);
}

int nmi_level_create_block(nmi_ctx *ctx, const float *d_xyz, const float *d_red, int64_t n_points, const uint8_t *d_frame, int32_t S_local,
                           int32_t s_offset, int32_t S_total, int32_t Wn_local, int32_t w_offset, int32_t Wn_total, float point_size,
                           nmi_level **out)
{
    return level_create(ctx, MapKind::points, d_xyz, d_red, n_points, nullptr, d_frame,
                        LevelBlock{S_local, s_offset, S_total, Wn_local, w_offset, Wn_total}, point_size, out);
}

int nmi_level_create_mesh_block(nmi_ctx *ctx, const float *d_xyz, const float *d_uv, int64_t n_triangles, const nmi_texture *tex,
                                const uint8_t *d_frame, int32_t S_local, int32_t s_offset, int32_t S_total, int32_t Wn_local,
                                int32_t w_offset, int32_t Wn_total, nmi_level **out)
{
    if (!tex) return NMI_ERR_INVALID_ARGUMENT;
    return level_create(ctx, MapKind::textured_mesh, d_xyz, d_uv, n_triangles, tex, d_frame,
                        LevelBlock{S_local, s_offset, S_total, Wn_local, w_offset, Wn_total}, 1.0f, out);
}

int nmi_level_create_mesh_colored_block(nmi_ctx *ctx, const float *d_xyz, const float *d_red, int64_t n_triangles, const uint8_t *d_frame,
                                        int32_t S_local, int32_t s_offset, int32_t S_total, int32_t Wn_local, int32_t w_offset,
                                        int32_t Wn_total, nmi_level **out)
{
    return level_create(ctx, MapKind::colored_mesh, d_xyz, d_red, n_triangles, nullptr, d_frame,
                        LevelBlock{S_local, s_offset, S_total, Wn_local, w_offset, Wn_total}, 1.0f, out);
}

}  // extern "C"

// Parameters of this replay into the pinned buffers the graph's first node reads; then the launch.  No waiting.
static int level_launch(nmi_level *lv, const float *h_mvps, const double *h_forward)
{
    nmi_ctx *ctx = lv->ctx;
    // every homography is checked before anything of the replay is touched: a rejected call leaves the level as it was
    std::vector<float> coeffs((size_t)lv->Wn * 9);
    for (int w = 0; w < lv->Wn; ++w)
        if (warp_inverse_coeffs(h_forward + (size_t)w * 9, coeffs.data() + (size_t)w * 9) != NMI_OK) return NMI_ERR_INVALID_ARGUMENT;
    float *own_mvps = lv->h_mvps.as<float>();
    memcpy(own_mvps, h_mvps, (size_t)lv->S * 16 * sizeof(float));
    nmi::level_views_bound(h_mvps, lv->S, own_mvps + (size_t)lv->S * 16);  // for the front kernel's first test: all views at once
    static const bool no_bound = getenv("NMI_LEVEL_NO_BOUND") != nullptr;      // measurement switch: six zero planes cull nothing
    if (no_bound) memset(own_mvps + (size_t)lv->S * 16, 0, 24 * sizeof(float));
    const uint32_t parity = ++lv->replay & 1u;  // which of its two counters the prep kernel's cull counts under (it zeroes the other one)
    memcpy(own_mvps + (size_t)lv->S * 16 + 24, &parity, sizeof parity);
    memcpy(lv->h_coeffs.as<>(), coeffs.data(), coeffs.size() * sizeof(float));
    constexpr unsigned long long kPending = ~0ull;
    __atomic_store_n(lv->h_key.as<unsigned long long>(), kPending, __ATOMIC_RELEASE);
    const hipError_t le = hipGraphLaunch(lv->exec, ctx->stream);
    if (le != hipSuccess) {
        --lv->replay;  // (the replay did not run: its counter has not been counted into, the other one has not been zeroed)
        return hip_fail(ctx, le, "hipGraphLaunch");
    }
    return NMI_OK;
}

// nmi_level_run_rccl's device side (nmi_capi_rccl.cpp): replay the block's graph (if the block is not empty) and hand back the
// device word that holds this rank's key once the context's stream has reached this point.
int nmi_internal::level_enqueue(nmi_level *lv, const float *h_mvps, const double *h_forward, const unsigned long long **d_key)
{
    if (!lv || !d_key) return NMI_ERR_INVALID_ARGUMENT;
    *d_key = lv->d_key.as<unsigned long long>();
    if (lv->S == 0 || lv->Wn == 0) return NMI_OK;  // d_key holds 0 = "no candidate" since creation
    if (!h_mvps || !h_forward) return NMI_ERR_INVALID_ARGUMENT;
    lv->ctx->detail.clear();
    return level_launch(lv, h_mvps, h_forward);
}

nmi_ctx *nmi_internal::level_ctx(nmi_level *lv) { return lv ? lv->ctx : nullptr; }

extern "C" {

int nmi_level_run(nmi_level *lv, const float *h_mvps, const double *h_forward, int64_t *h_best_index, float *h_best_score)
{
    if (!lv) return NMI_ERR_INVALID_ARGUMENT;
    if (lv->S == 0 || lv->Wn == 0) return nmi_key_unpack(0, h_best_index, h_best_score);  // empty block: no candidate
    if (!h_mvps || !h_forward) return NMI_ERR_INVALID_ARGUMENT;
    nmi_ctx *ctx = lv->ctx;
    ctx->detail.clear();
    DeviceGuard guard(ctx->device);
    // the previous replay has completed (this call is blocking), so the pinned parameter buffers are free to rewrite.
    // The search kernel's last workgroup stores the winner (never all ones: scores are non-negative floats) into
    // *h_key with system scope; polling that word returns ~10 us earlier than waiting for the stream to drain.
    constexpr unsigned long long kPending = ~0ull;
    const int lrc = level_launch(lv, h_mvps, h_forward);
    if (lrc != NMI_OK) return lrc;
    const unsigned long long *h_key = lv->h_key.as<unsigned long long>();
    unsigned long long key = kPending;
    for (uint64_t spin = 0; key == kPending; ++spin) {
        key = __atomic_load_n(h_key, __ATOMIC_ACQUIRE);
        if (key == kPending && (spin & 0xFFFF) == 0xFFFF) {
            const hipError_t q = hipStreamQuery(ctx->stream);  // a faulted or finished stream must not leave us spinning
            if (q == hipSuccess) {
                key = __atomic_load_n(h_key, __ATOMIC_ACQUIRE);
                break;
            }
            if (q != hipErrorNotReady) return hip_fail(ctx, q, "hipStreamQuery");
        }
    }
    if (key == kPending) return NMI_ERR_HIP;  // the graph ran without posting: cannot happen with a non-empty grid
    return nmi_key_unpack(key, h_best_index, h_best_score);
}

int nmi_level_copy_outputs(nmi_level *lv, uint8_t *h_renders, uint8_t *h_warps, float *h_ratings)
{
    if (!lv) return NMI_ERR_INVALID_ARGUMENT;
    nmi_ctx *ctx = lv->ctx;
    if (lv->S == 0 || lv->Wn == 0) return NMI_OK;  // empty block: nothing was produced
    DeviceGuard guard(ctx->device);
    NMI_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // nmi_level_run returns when the winner is posted, a little before the graph has drained
    const size_t npix = (size_t)ctx->npix;
    if (h_renders) NMI_HIP_TRY(ctx, hipMemcpy(h_renders, lv->d_renders.as<>(), npix * lv->S, hipMemcpyDeviceToHost));
    if (h_warps) NMI_HIP_TRY(ctx, hipMemcpy(h_warps, lv->d_warps.as<>(), npix * lv->Wn, hipMemcpyDeviceToHost));
    if (h_ratings) NMI_HIP_TRY(ctx, hipMemcpy(h_ratings, lv->d_ratings.as<>(), (size_t)lv->S * lv->Wn * sizeof(float), hipMemcpyDeviceToHost));
    return NMI_OK;
}

int nmi_level_set_masks(nmi_level *lv, int32_t enabled, const uint8_t *d_frame_mask)
{
    if (!lv || (enabled != 0 && enabled != 1) || (!enabled && d_frame_mask)) return NMI_ERR_INVALID_ARGUMENT;
    if (lv->set.covered) return NMI_ERR_INVALID_ARGUMENT;  // a covered level turns coverage off first (nmi_level_set_coverage)
    LevelSettings next = lv->set;
    next.masked = enabled != 0;
    next.d_frame_mask = d_frame_mask;
    return level_apply(lv, next, "nmi_level_set_masks", next.masked);
}

int nmi_level_copy_masks(nmi_level *lv, uint8_t *h_warp_masks, int32_t *h_counts)
{
    if (!lv || !lv->set.masked) return NMI_ERR_INVALID_ARGUMENT;
    if (lv->S == 0 || lv->Wn == 0) return NMI_OK;  // empty block: nothing was produced
    nmi_ctx *ctx = lv->ctx;
    DeviceGuard guard(ctx->device);
    NMI_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (h_warp_masks) NMI_HIP_TRY(ctx, hipMemcpy(h_warp_masks, lv->d_masks.as<>(), (size_t)ctx->npix * lv->Wn, hipMemcpyDeviceToHost));
    if (h_counts) NMI_HIP_TRY(ctx, hipMemcpy(h_counts, lv->d_counts.as<>(), (size_t)lv->Wn * sizeof(int32_t), hipMemcpyDeviceToHost));
    return NMI_OK;
}

int nmi_level_set_coverage(nmi_level *lv, int32_t enabled, const uint8_t *d_frame_mask)
{
    if (!lv || (enabled != 0 && enabled != 1) || (!enabled && d_frame_mask)) return NMI_ERR_INVALID_ARGUMENT;
    if (lv->set.masked) return NMI_ERR_INVALID_ARGUMENT;  // a masked level turns its masks off first (nmi_level_set_masks)
    LevelSettings next = lv->set;
    next.covered = enabled != 0;
    next.d_frame_mask = d_frame_mask;
    return level_apply(lv, next, "nmi_level_set_coverage");
}

int nmi_level_copy_coverage(nmi_level *lv, uint8_t *h_render_masks, uint8_t *h_warp_masks, int32_t *h_counts)
{
    if (!lv || !lv->set.covered) return NMI_ERR_INVALID_ARGUMENT;
    if (lv->S == 0 || lv->Wn == 0) return NMI_OK;  // empty block: nothing was produced
    nmi_ctx *ctx = lv->ctx;
    DeviceGuard guard(ctx->device);
    NMI_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    const size_t npix = (size_t)ctx->npix;
    if (h_render_masks) NMI_HIP_TRY(ctx, hipMemcpy(h_render_masks, lv->d_rmasks.as<>(), npix * lv->S, hipMemcpyDeviceToHost));
    if (h_warp_masks) NMI_HIP_TRY(ctx, hipMemcpy(h_warp_masks, lv->d_masks.as<>(), npix * lv->Wn, hipMemcpyDeviceToHost));
    if (h_counts) NMI_HIP_TRY(ctx, hipMemcpy(h_counts, lv->d_cover_counts.as<>(), (size_t)lv->S * lv->Wn * sizeof(int32_t), hipMemcpyDeviceToHost));
    return NMI_OK;
}

int nmi_level_set_distortion(nmi_level *lv, const double K[9], const float dist[5])
{
    // A bad K or dist is refused without reading *lv, as by nmi_stream_set_distortion (tests/test_undistort_api.py calls both
    // with a handle that is not a level's): checked on a value of its own first, then set on the copy of the level's settings.
    FrameIntake probe;
    if (!lv || intake_set_distortion(&probe, K, dist) != NMI_OK) return NMI_ERR_INVALID_ARGUMENT;
    LevelSettings next = lv->set;
    (void)intake_set_distortion(&next.intake, K, dist);
    return level_apply(lv, next, "nmi_level_set_distortion");
}

int nmi_level_set_distortion_fisheye(nmi_level *lv, const double K[9], const double K_raw[9], const float dist[4])
{
    FrameIntake probe;  // (as nmi_level_set_distortion: a bad argument is refused without reading *lv)
    if (!lv || intake_set_distortion_fisheye(&probe, K, K_raw, dist) != NMI_OK) return NMI_ERR_INVALID_ARGUMENT;
    LevelSettings next = lv->set;
    (void)intake_set_distortion_fisheye(&next.intake, K, K_raw, dist);
    return level_apply(lv, next, "nmi_level_set_distortion_fisheye");
}

// nmi_level_set_frame_format is nmi_level_set_frame_reduction with factor 1: one setting, the later call wins.
int nmi_level_set_frame_reduction(nmi_level *lv, int32_t factor, int32_t format, int64_t pitch)
{
    if (!lv) return NMI_ERR_INVALID_ARGUMENT;
    LevelSettings next = lv->set;
    if (intake_set_frame(&next.intake, lv->ctx->params.width, lv->ctx->params.height, factor, format, pitch) != NMI_OK) return NMI_ERR_INVALID_ARGUMENT;
    if (!frame_base_ok(format, lv->d_frame)) return NMI_ERR_INVALID_ARGUMENT;
    return level_apply(lv, next, "nmi_level_set_frame_reduction");
}

int nmi_level_set_tone_map(nmi_level *lv, const nmi_tone_map *tm)
{
    FrameIntake probe;
    if (!lv || intake_set_tone_map(&probe, lv->ctx->params.width, lv->ctx->params.height, tm) != NMI_OK) return NMI_ERR_INVALID_ARGUMENT;
    LevelSettings next = lv->set;
    next.intake.tone = probe.tone;
    return level_apply(lv, next, "nmi_level_set_tone_map");
}

int nmi_level_set_valid_range(nmi_level *lv, int32_t lo, int32_t hi)
{
    FrameIntake probe;
    if (!lv || intake_set_valid_range(&probe, lo, hi) != NMI_OK) return NMI_ERR_INVALID_ARGUMENT;
    LevelSettings next = lv->set;
    next.intake.valid = probe.valid;
    return level_apply(lv, next, "nmi_level_set_valid_range");
}

int nmi_level_set_depth_shade(nmi_level *lv, const nmi_depth_shade *shade)
{
    nmi::DepthShade sh{};
    if (!lv || (shade ? depth_shade_check(shade, &sh) != NMI_OK : lv->no_attr)) return NMI_ERR_INVALID_ARGUMENT;
    LevelSettings next = lv->set;
    next.depth = shade != nullptr;
    next.shade = sh;
    return level_apply(lv, next, "nmi_level_set_depth_shade");
}

int nmi_level_set_frame_format(nmi_level *lv, int32_t format, int64_t pitch) { return nmi_level_set_frame_reduction(lv, 1, format, pitch); }

int nmi_level_set_peaks(nmi_level *lv, int32_t K, const int32_t num[6], const int32_t radius[6])
{
    if (!lv || K < 0 || K > nmi::kPeaksMaxK || (K > 0 && (!num || !radius))) return NMI_ERR_INVALID_ARGUMENT;
    nmi::PeaksArgs pk{};
    if (K > 0) {
        const int shape = nmi::peaks_shape(num, radius, pk);
        if (shape == -1) return NMI_ERR_INVALID_ARGUMENT;
        // greedy suppression over a block is not the suppression of the whole grid
        if (lv->S != lv->S_total || lv->Wn != lv->Wn_total) return NMI_ERR_UNSUPPORTED;
        if ((int64_t)num[0] * num[1] * num[2] != lv->S || (int64_t)num[3] * num[4] * num[5] != lv->Wn) return NMI_ERR_INVALID_ARGUMENT;
        if (shape != 0) return NMI_ERR_UNSUPPORTED;
        pk.K = K;
    }
    LevelSettings next = lv->set;
    next.peaks = pk;
    if (K == 0) next.refine = false;  // nothing to refine
    return level_apply(lv, next, "nmi_level_set_peaks");
}

int nmi_level_copy_peaks(nmi_level *lv, uint64_t *h_keys, int32_t *h_count)
{
    if (!lv || lv->set.peaks.K < 1 || (!h_keys && !h_count)) return NMI_ERR_INVALID_ARGUMENT;
    nmi_ctx *ctx = lv->ctx;
    DeviceGuard guard(ctx->device);
    NMI_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // nmi_level_run returns at the winner, before the peaks node has run
    const int K = lv->set.peaks.K;
    uint64_t keys[nmi::kPeaksMaxK];
    NMI_HIP_TRY(ctx, hipMemcpy(keys, lv->d_peaks.as<>(), (size_t)K * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (h_keys) memcpy(h_keys, keys, (size_t)K * sizeof(uint64_t));
    if (h_count) {
        int32_t n = 0;
        while (n < K && keys[n] != 0) ++n;
        *h_count = n;
    }
    return NMI_OK;
}

int nmi_level_set_refine(nmi_level *lv, int32_t on)
{
    if (!lv) return NMI_ERR_INVALID_ARGUMENT;
    if (lv->S != lv->S_total || lv->Wn != lv->Wn_total) return NMI_ERR_UNSUPPORTED;  // as the peaks of a block
    if (lv->set.peaks.K < 1) return NMI_ERR_INVALID_ARGUMENT;
    LevelSettings next = lv->set;
    next.refine = on != 0;
    return level_apply(lv, next, "nmi_level_set_refine");
}

int nmi_level_copy_refined(nmi_level *lv, nmi_refined_peak *h_records, int32_t *h_count)
{
    if (!lv || !lv->set.refine || (!h_records && !h_count)) return NMI_ERR_INVALID_ARGUMENT;
    nmi_ctx *ctx = lv->ctx;
    DeviceGuard guard(ctx->device);
    NMI_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // nmi_level_run returns at the winner, before these nodes have run
    const int K = lv->set.peaks.K;
    nmi_refined_peak records[nmi::kRefineMaxK];
    NMI_HIP_TRY(ctx, hipMemcpy(records, lv->d_refined.as<>(), (size_t)K * sizeof(nmi_refined_peak), hipMemcpyDeviceToHost));
    if (h_records) memcpy(h_records, records, (size_t)K * sizeof(nmi_refined_peak));
    if (h_count) {
        int32_t n = 0;
        while (n < K && records[n].key != 0) ++n;  // (empty records follow the peaks: none in between)
        *h_count = n;
    }
    return NMI_OK;
}

// ---------------------------------------------------------------------------------------------------------
// Streaming pipeline (config 5): double-buffered render stacks, copy stream beside the compute stream.
// ---------------------------------------------------------------------------------------------------------
}  // extern "C"

struct nmi_stream {
    nmi_ctx *ctx = nullptr;
    int depth = 0, max_S = 0, max_Wn = 0;
    nmi_mem::Stream copy;
    struct Slot {
        DeviceBuffer d_renders;      // uint8_t [max_S][H][W]
        DeviceBuffer d_ratings;      // float [max_Wn][max_S], only with nmi_stream_keep_ratings
        int S = 0, Wn = 0;           // grid of the slot's latest submission
        DeviceBuffer d_key;          // unsigned long long [2]: this rank's key, and the all-reduced one (block submissions with a communicator)
        PinnedBuffer h_key;          // unsigned long long
        nmi_mem::Event copied, done;
        int64_t ticket = -1;
        bool waited = true;
        bool failed = false;         // its search timed out in the split kernel and could not be redone (nmi_stream_wait)
        SearchLaunch launch;         // the slot's launch: it answers for itself (split form, epoch) when the ticket is waited
                                     //   for, whatever was launched after it
        int s_offset = 0, S_total = 0, w_offset = 0;  // position of the slot's block in its level
        int warp_buf = 0;            // warp buffer the search read, and that buffer's generation at submission
        uint64_t warp_gen = 0;
        // masked / covered tickets (allocated on the stream's first such submission, see nmi_stream_submit_masked)
        int kind = 0;                // kPlain, kMasked, kCovered
        int64_t n_counts = 0;        // entries of d_counts the ticket wrote: len_w [Wn] (masked), len [Wn][S] (covered)
        DeviceBuffer d_counts;       // int32_t [max_Wn * max_S]
        DeviceBuffer d_bits;         // uint8_t [max_S][ceil(npix / 8)]: the render-mask bits, uploaded beside the render stack (covered)
    };
    std::vector<Slot> slots;   // [depth]
    DeviceBuffer d_frame[2];   // uint8_t [H][W]: frames alternate so an upload never overwrites one still being warped
    DeviceBuffer d_warps[2];   // uint8_t [max_Wn][H][W]
    nmi_mem::Event frame_copied, warps_free[2];
    int warp_buf = 0;      // buffer holding the current warp stack
    uint64_t warp_gen[2] = {0, 0};  // refills of each warp buffer so far
    int cur_Wn = 0;
    bool have_warps = false;
    bool keep_ratings = false;
    int64_t next_ticket = 0;
    // Masks, beside the warp buffers: the frame mask and the warp masks of each buffer's frame, and -- for masked tickets --
    // len_w and the per-warp term tables, built once per frame submission (a frame-less ticket reuses them).
    DeviceBuffer d_fmask[2];                      // uint8_t [H][W]
    DeviceBuffer d_wmasks[2];                     // uint8_t [max_Wn][H][W]
    DeviceBuffer d_wcounts[2];                    // int32_t [max_Wn]
    DeviceBuffer d_wtables[2];                    // float [max_Wn][npix + 1]
    bool masks_ok[2] = {false, false};            // the buffer's frame was submitted masked or covered: its warp masks exist
    bool tables_ok[2] = {false, false};           // ... and its len_w / tables have been built
    // Unpacked render masks of the covered ticket being searched.  ONE buffer for all slots: the unpack and the search that
    // reads it both run on the context's compute stream, so ticket i + 1's unpack cannot start before ticket i's search ended.
    DeviceBuffer d_rmasks;                        // uint8_t [max_S][H][W]
    DeviceBuffer d_redo;                          // int32_t [max_S * max_Wn] redo list of the optimistic masked / covered launch (stream-ordered too)
    DeviceBuffer d_redo_state;                    // uint32_t [2], zero between searches
    // The frame's way in (nmi_stream_set_distortion, _set_frame_format, _set_frame_reduction; with them the tone map and the valid
    // range of a deep frame, nmi_stream_set_tone_map, _set_valid_range): frames submitted while one of the former
    // is set are brought on the compute stream into d_ud[b] (distorted, masked / covered: their masks into d_ud_mask[b]), and the
    // warps are made from those.  A coloured, pitched or full-size host frame (intake.colored) crosses as its rows of
    // intake.frame_pitch bytes into the dense colour slot d_color[b]; reduced (or a Bayer mosaic, or deep) and distorted, it is brought to
    // grey in d_frame[b] (idle meanwhile), which the undistortion reads as a grey frame.
    FrameIntake intake;
    DeviceBuffer d_ud[2];                         // uint8_t [H][W], allocated on the first distorted (or coloured) frame
    DeviceBuffer d_ud_mask[2];                    // uint8_t [H][W], allocated on the first distorted masked / covered frame
    DeviceBuffer d_color[2];                      // [f H][f W * bytes per pixel], allocated on the first coloured frame, grown for a larger one
    ToneWork tone_work;                           // deep frames (GRAY16): one histogram and table, used in turn on the compute stream
};

namespace {

enum { kPlain = 0, kMasked = 1, kCovered = 2 };

// Buffers of masked / covered tickets, allocated on the stream's first such submission (a plain-only stream never has them).
// Each buffer has one size and is allocated once (a grow that fits is no call at all); after a failure the next submission
// allocates what is still missing.
int stream_alloc_masks(nmi_stream *st, int kind)
{
    nmi_ctx *ctx = st->ctx;
    const size_t npix = (size_t)ctx->npix, cells = (size_t)st->max_S * st->max_Wn;
    for (int b = 0; b < 2; ++b) {
        NMI_HIP_TRY(ctx, st->d_fmask[b].grow(npix));
        NMI_HIP_TRY(ctx, st->d_wmasks[b].grow(npix * st->max_Wn));
    }
    for (nmi_stream::Slot &s : st->slots) NMI_HIP_TRY(ctx, s.d_counts.grow(cells * sizeof(int32_t)));
    NMI_HIP_TRY(ctx, st->d_redo.grow(cells * sizeof(int32_t)));
    NMI_HIP_TRY(ctx, st->d_redo_state.grow(2 * sizeof(uint32_t), ctx->stream, /*zero=*/true));
    if (kind == kMasked) {
        for (int b = 0; b < 2; ++b) {
            NMI_HIP_TRY(ctx, st->d_wcounts[b].grow((size_t)st->max_Wn * sizeof(int32_t)));
            NMI_HIP_TRY(ctx, st->d_wtables[b].grow((size_t)st->max_Wn * (npix + 1) * sizeof(float)));
        }
    }
    if (kind == kCovered) {
        for (nmi_stream::Slot &s : st->slots) NMI_HIP_TRY(ctx, s.d_bits.grow(nmi::mask_bit_bytes(ctx->npix) * st->max_S));
        NMI_HIP_TRY(ctx, st->d_rmasks.grow(npix * st->max_S));
    }
    return NMI_OK;
}

}  // namespace

extern "C" {

int nmi_stream_destroy(nmi_stream *st)
{
    if (!st) return NMI_OK;
    DeviceGuard guard(st->ctx->device);
    (void)hipStreamSynchronize(st->ctx->stream);
    if (st->copy) (void)hipStreamSynchronize(st->copy);
    delete st;
    return NMI_OK;
}

int nmi_stream_create(nmi_ctx *ctx, int32_t max_S, int32_t max_Wn, int32_t depth, nmi_stream **out)
{
    if (!ctx || !out || max_S <= 0 || max_Wn <= 0 || depth < 2 || depth > 64) return NMI_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    DeviceGuard guard(ctx->device);
    nmi_stream *st = new (std::nothrow) nmi_stream;
    if (!st) return NMI_ERR_INVALID_ARGUMENT;
    st->ctx = ctx;
    st->depth = depth;
    st->max_S = max_S;
    st->max_Wn = max_Wn;
    st->slots = std::vector<nmi_stream::Slot>(depth);
    const size_t npix = (size_t)ctx->npix;
    FirstError ok;
    ok(st->copy.create(hipStreamNonBlocking));
    for (nmi_stream::Slot &s : st->slots) {
        if (ok.e != hipSuccess) break;
        ok(s.d_renders.alloc(npix * max_S));
        ok(s.d_key.alloc(2 * sizeof(unsigned long long)));
        ok(s.h_key.alloc(sizeof(unsigned long long), nmi_mem::kPinned));
        ok(s.copied.create(hipEventDisableTiming));
        ok(s.done.create(hipEventDisableTiming));
    }
    for (int b = 0; b < 2 && ok.e == hipSuccess; ++b) {
        ok(st->d_frame[b].alloc(npix));
        ok(st->d_warps[b].alloc(npix * max_Wn));
        ok(st->warps_free[b].create(hipEventDisableTiming));
    }
    ok(st->frame_copied.create(hipEventDisableTiming));
    if (ok.e != hipSuccess) {
        const int rc = hip_fail(ctx, ok.e, "nmi_stream_create");
        nmi_stream_destroy(st);
        return rc;
    }
    *out = st;
    return NMI_OK;
}

int nmi_stream_submit(nmi_stream *st, const uint8_t *h_render_stack, int32_t S, const uint8_t *h_frame,
                      const double *h_forward, int32_t Wn, int64_t *ticket)
{
    if (S <= 0) return NMI_ERR_INVALID_ARGUMENT;
    return nmi_stream_submit_block(st, h_render_stack, S, 0, S, h_frame, h_forward, Wn, 0, h_frame ? Wn : (st ? st->cur_Wn : 0), nullptr, ticket);
}

}  // extern "C"

// Every submission form.  kind kPlain is nmi_stream_submit_block as it always was; kMasked / kCovered add the masks and take the
// masked / covered search (never the split kernel: launch.parts stays 0, so nmi_stream_wait never redoes them).
static int stream_submit(nmi_stream *st, int kind, const uint8_t *h_render_stack, const uint8_t *h_bits, int32_t S, int32_t s_offset,
                         int32_t S_total, const uint8_t *h_frame, const uint8_t *h_frame_mask, const double *h_forward, int32_t Wn,
                         int32_t w_offset, int32_t Wn_total, void *nccl_comm, int64_t *ticket)
{
    if (!st || !ticket || S < 0 || S > st->max_S || (S > 0 && !h_render_stack)) return NMI_ERR_INVALID_ARGUMENT;
    if (h_frame && (!h_forward || Wn <= 0 || Wn > st->max_Wn)) return NMI_ERR_INVALID_ARGUMENT;
    if (!h_frame && !st->have_warps && !(S == 0 && nccl_comm)) return NMI_ERR_INVALID_ARGUMENT;
    if (h_frame_mask && !h_frame) return NMI_ERR_INVALID_ARGUMENT;                      // a frame mask goes with its frame
    if (kind == kCovered && S > 0 && !h_bits) return NMI_ERR_INVALID_ARGUMENT;         // never the masked search in disguise
    // frame-less masked / covered: the most recent frame must have been submitted with masks (a plain one made none)
    if (kind != kPlain && !h_frame && st->have_warps && !st->masks_ok[st->warp_buf]) return NMI_ERR_INVALID_ARGUMENT;
    const int32_t Wn_block = h_frame ? Wn : st->cur_Wn;
    if (s_offset < 0 || w_offset < 0 || s_offset + S > S_total || w_offset + Wn_block > Wn_total) return NMI_ERR_INVALID_ARGUMENT;
    if ((int64_t)S_total * Wn_total >= 0x7FFFFFFFll) return NMI_ERR_UNSUPPORTED;
    nmi_ctx *ctx = st->ctx;
    ctx->detail.clear();
    DeviceGuard guard(ctx->device);
    const int64_t t = st->next_ticket;
    nmi_stream::Slot &s = st->slots[t % st->depth];
    if (!s.waited) return NMI_ERR_NOT_READY;  // the ticket that used this slot has not been collected yet
    const size_t npix = (size_t)ctx->npix;
    if (kind != kPlain) {
        const int rc = stream_alloc_masks(st, kind);
        if (rc != NMI_OK) return rc;
    }
    const FrameIntake in = st->intake;  // (this submission's: a later setter call does not reach it)
    const bool undistort = h_frame && in.distorted, colored = h_frame && in.colored;
    const int32_t factor = in.frame_factor;
    const int64_t dense_row = frame_row_bytes(in.frame_format, (int64_t)factor * ctx->params.width);  // (packed: 10 or 12 bits per pixel)
    const size_t color_rows = (size_t)factor * ctx->params.height, color_need = (size_t)dense_row * color_rows;
    for (int b = 0; (undistort || colored) && b < 2; ++b) {
        NMI_HIP_TRY(ctx, st->d_ud[b].grow(npix));
        if (undistort && kind != kPlain) NMI_HIP_TRY(ctx, st->d_ud_mask[b].grow(npix));
    }
    if (colored && st->d_color[1].size() < color_need) {  // (a wider format or a larger frame than the slots were made for; [1] is allocated last)
        NMI_HIP_TRY(ctx, hipStreamSynchronize(st->copy));        // nothing in flight reads or fills the old slots
        NMI_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        for (int b = 0; b < 2; ++b) NMI_HIP_TRY(ctx, st->d_color[b].grow(color_need));
    }

    // typed views of the slot's and the stream's buffers (a masked or covered ticket's: null on a stream that has had none)
    uint8_t *d_renders = s.d_renders.as<uint8_t>(), *d_bits = s.d_bits.as<uint8_t>(), *d_rmasks = st->d_rmasks.as<uint8_t>();
    unsigned long long *d_key = s.d_key.as<unsigned long long>();
    int32_t *d_counts = s.d_counts.as<int32_t>(), *d_redo = st->d_redo.as<int32_t>();
    uint32_t *d_redo_state = st->d_redo_state.as<uint32_t>();

    // copy stream: render stack of this level into the slot (the slot's previous search finished: it was waited for)
    if (S > 0) NMI_HIP_TRY(ctx, hipMemcpyAsync(d_renders, h_render_stack, npix * S, hipMemcpyHostToDevice, st->copy));
    if (kind == kCovered && S > 0)  // its coverage as bits: 1/8 of the render stack's bytes on the wire
        NMI_HIP_TRY(ctx, hipMemcpyAsync(d_bits, h_bits, nmi::mask_bit_bytes(ctx->npix) * S, hipMemcpyHostToDevice, st->copy));
    if (h_frame) {
        const int nb = st->have_warps ? st->warp_buf ^ 1 : 0;
        uint8_t *d_frame = st->d_frame[nb].as<uint8_t>(), *d_fmask = st->d_fmask[nb].as<uint8_t>(), *d_color = st->d_color[nb].as<uint8_t>();
        uint8_t *d_ud = st->d_ud[nb].as<uint8_t>(), *d_warps = st->d_warps[nb].as<uint8_t>(), *d_wmasks = st->d_wmasks[nb].as<uint8_t>();
        // the buffer being refilled was last read by searches submitted before the previous frame switch
        NMI_HIP_TRY(ctx, hipStreamWaitEvent(st->copy, st->warps_free[nb], 0));
        if (colored)  // the rows of the host's pitch (H of them, or f H) into the dense colour slot
            NMI_HIP_TRY(ctx, hipMemcpy2DAsync(d_color, (size_t)dense_row, h_frame, (size_t)in.frame_pitch, (size_t)dense_row, color_rows,
                                              hipMemcpyHostToDevice, st->copy));
        else
            NMI_HIP_TRY(ctx, hipMemcpyAsync(d_frame, h_frame, npix, hipMemcpyHostToDevice, st->copy));
        if (h_frame_mask) NMI_HIP_TRY(ctx, hipMemcpyAsync(d_fmask, h_frame_mask, npix, hipMemcpyHostToDevice, st->copy));
        NMI_HIP_TRY(ctx, hipEventRecord(st->frame_copied, st->copy));
        NMI_HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, st->frame_copied, 0));
        if (st->have_warps) NMI_HIP_TRY(ctx, hipEventRecord(st->warps_free[st->warp_buf], ctx->stream));
        const uint8_t *frame = d_frame, *frame_mask = h_frame_mask ? d_fmask : nullptr;
        // the camera's frame (and mask) -> the grey, undistorted ones, on the compute stream: the warps read them next
        uint8_t *ud_mask = undistort && kind != kPlain ? st->d_ud_mask[nb].as<uint8_t>() : nullptr;
        // A deep frame under a valid range, masked or covered: the conversion writes validity into the frame-mask slot, in place
        // over an uploaded h_frame_mask.  The slot is now written on the compute stream; the copy stream's next upload into it
        // still waits for warps_free[nb], recorded on the compute stream behind this frame's conversion (at the next frame switch).
        uint8_t *valid = kind != kPlain && in.validity() ? d_fmask : nullptr;
        if (in.deep()) NMI_HIP_TRY(ctx, tone_prepare(&st->tone_work, in.tone, ctx->stream, in.container(ctx->params.width, ctx->params.height)));
        NMI_HIP_TRY(ctx, launch_intake(in, st->tone_work, colored ? d_color : d_frame, dense_row, frame_mask, d_frame, d_ud, ud_mask,
                                       valid, ctx->params.width, ctx->params.height, ctx->stream));
        if (in.own_frame()) frame = d_ud;
        if (valid) frame_mask = valid;
        if (undistort) frame_mask = ud_mask;
        int rc = kind == kPlain ? nmi_warp_stack(ctx, frame, h_forward, Wn, d_warps)
                                : nmi_warp_stack_masked(ctx, frame, frame_mask, h_forward, Wn, d_warps, d_wmasks);
        if (rc != NMI_OK) return rc;
        st->warp_buf = nb;
        ++st->warp_gen[nb];
        st->cur_Wn = Wn;
        st->have_warps = true;
        st->masks_ok[nb] = kind != kPlain;
        st->tables_ok[nb] = false;
    }
    const int wb = st->warp_buf;
    uint8_t *d_warps = st->d_warps[wb].as<uint8_t>(), *d_wmasks = st->d_wmasks[wb].as<uint8_t>();
    int32_t *d_wcounts = st->d_wcounts[wb].as<int32_t>();
    float *d_wtables = st->d_wtables[wb].as<float>();
    if (kind == kMasked && st->have_warps && !st->tables_ok[wb]) {
        // len_w and the per-warp term tables of this buffer's warp masks: once per frame (nmi_search_grid_masked's kernels)
        NMI_HIP_TRY(ctx, nmi::launch_mask_counts(d_wmasks, st->cur_Wn, ctx->npix, d_wcounts, ctx->stream));
        NMI_HIP_TRY(ctx, nmi::launch_mask_tables(d_wcounts, st->cur_Wn, ctx->npix, d_wtables, ctx->stream));
        st->tables_ok[wb] = true;
    }
    NMI_HIP_TRY(ctx, hipEventRecord(s.copied, st->copy));

    // compute stream: search on the slot, winner to pinned host memory
    NMI_HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, s.copied, 0));
    if (st->keep_ratings) NMI_HIP_TRY(ctx, s.d_ratings.grow((size_t)st->max_S * st->max_Wn * sizeof(float)));
    s.S = S;
    s.Wn = st->cur_Wn;
    s.s_offset = s_offset;
    s.S_total = S_total;
    s.w_offset = w_offset;
    int rc = NMI_OK;
    SearchRequest rq = SearchRequest::block(d_renders, S, s_offset, S_total, d_warps, st->cur_Wn, w_offset);
    rq.d_ratings = st->keep_ratings ? s.d_ratings.as<float>() : nullptr;
    rq.out_key = d_key;
    if (kind == kPlain || (int64_t)S * st->cur_Wn == 0) {
        // nmi_stream_wait checks this very launch for a split-kernel timeout (s.launch) and redoes it -- which it cannot
        // do once the key has gone into a collective, so submissions with a communicator keep to the one-workgroup kernel.
        // (An empty masked / covered block comes here too: nothing is scored, the key is "none".)
        rq.caller_checks_split = nccl_comm == nullptr && kind == kPlain;
        rc = enqueue_grid(ctx, rq, &s.launch);
    } else if (kind == kMasked) {
        rc = enqueue_grid_mask(ctx, rq, MaskSide{d_wmasks, nullptr, d_wcounts, d_wtables, d_redo, d_redo_state}, &s.launch);
    } else {
        NMI_HIP_TRY(ctx, nmi::launch_unpack_mask_bits(d_bits, S, ctx->npix, d_rmasks, ctx->stream));
        rc = enqueue_grid_mask(ctx, rq, MaskSide{d_wmasks, d_rmasks, d_counts, nullptr, d_redo, d_redo_state}, &s.launch);
    }
    if (rc != NMI_OK) return rc;
    s.kind = kind;
    s.n_counts = kind == kMasked ? st->cur_Wn : kind == kCovered ? (int64_t)S * st->cur_Wn : 0;
    if (kind == kMasked && s.n_counts > 0)  // len_w into the slot: the buffer's own may be rebuilt by a later frame
        NMI_HIP_TRY(ctx, hipMemcpyAsync(d_counts, d_wcounts, (size_t)s.n_counts * sizeof(int32_t), hipMemcpyDeviceToDevice, ctx->stream));
    s.warp_buf = wb;
    s.warp_gen = st->warp_gen[wb];
    const unsigned long long *result = d_key;
    if (nccl_comm) {
        // the level's only exchange: 8-byte MAX all-reduce of the packed keys, issued in submission order on every rank
        rc = rccl_allreduce_key(ctx, d_key, d_key + 1, nccl_comm);
        if (rc != NMI_OK) return rc;
        result = d_key + 1;
    }
    NMI_HIP_TRY(ctx, hipMemcpyAsync(s.h_key.as<>(), result, sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    NMI_HIP_TRY(ctx, hipEventRecord(s.done, ctx->stream));
    s.ticket = t;
    s.waited = false;
    s.failed = false;
    *ticket = t;
    ++st->next_ticket;
    return NMI_OK;
}

extern "C" {

int nmi_stream_submit_block(nmi_stream *st, const uint8_t *h_render_stack, int32_t S, int32_t s_offset, int32_t S_total,
                            const uint8_t *h_frame, const double *h_forward, int32_t Wn, int32_t w_offset, int32_t Wn_total,
                            void *nccl_comm, int64_t *ticket)
{
    return stream_submit(st, kPlain, h_render_stack, nullptr, S, s_offset, S_total, h_frame, nullptr, h_forward, Wn, w_offset, Wn_total,
                         nccl_comm, ticket);
}

int nmi_stream_submit_masked(nmi_stream *st, const uint8_t *h_render_stack, int32_t S, const uint8_t *h_frame, const uint8_t *h_frame_mask,
                             const double *h_forward, int32_t Wn, int64_t *ticket)
{
    if (S <= 0) return NMI_ERR_INVALID_ARGUMENT;
    return stream_submit(st, kMasked, h_render_stack, nullptr, S, 0, S, h_frame, h_frame_mask, h_forward, Wn, 0,
                         h_frame ? Wn : (st ? st->cur_Wn : 0), nullptr, ticket);
}

int nmi_stream_submit_masked_block(nmi_stream *st, const uint8_t *h_render_stack, int32_t S_local, int32_t s_offset, int32_t S_total,
                                   const uint8_t *h_frame, const uint8_t *h_frame_mask, const double *h_forward, int32_t Wn_local,
                                   int32_t w_offset, int32_t Wn_total, void *nccl_comm, int64_t *ticket)
{
    return stream_submit(st, kMasked, h_render_stack, nullptr, S_local, s_offset, S_total, h_frame, h_frame_mask, h_forward, Wn_local,
                         w_offset, Wn_total, nccl_comm, ticket);
}

int nmi_stream_submit_covered(nmi_stream *st, const uint8_t *h_render_stack, const uint8_t *h_render_mask_bits, int32_t S,
                              const uint8_t *h_frame, const uint8_t *h_frame_mask, const double *h_forward, int32_t Wn, int64_t *ticket)
{
    if (S <= 0) return NMI_ERR_INVALID_ARGUMENT;
    return stream_submit(st, kCovered, h_render_stack, h_render_mask_bits, S, 0, S, h_frame, h_frame_mask, h_forward, Wn, 0,
                         h_frame ? Wn : (st ? st->cur_Wn : 0), nullptr, ticket);
}

int nmi_stream_submit_covered_block(nmi_stream *st, const uint8_t *h_render_stack, const uint8_t *h_render_mask_bits, int32_t S_local,
                                    int32_t s_offset, int32_t S_total, const uint8_t *h_frame, const uint8_t *h_frame_mask,
                                    const double *h_forward, int32_t Wn_local, int32_t w_offset, int32_t Wn_total, void *nccl_comm,
                                    int64_t *ticket)
{
    return stream_submit(st, kCovered, h_render_stack, h_render_mask_bits, S_local, s_offset, S_total, h_frame, h_frame_mask, h_forward,
                         Wn_local, w_offset, Wn_total, nccl_comm, ticket);
}

int nmi_stream_copy_counts(nmi_stream *st, int64_t ticket, int32_t *h_counts, int64_t n)
{
    if (!st || (!h_counts && n != 0) || ticket < 0 || ticket >= st->next_ticket) return NMI_ERR_INVALID_ARGUMENT;
    nmi_stream::Slot &s = st->slots[ticket % st->depth];
    // valid from nmi_stream_wait(ticket) until the slot is submitted to again; plain tickets have none
    if (s.ticket != ticket || !s.waited || s.failed || s.kind == kPlain || n != s.n_counts) return NMI_ERR_INVALID_ARGUMENT;
    if (n == 0) return NMI_OK;
    nmi_ctx *ctx = st->ctx;
    DeviceGuard guard(ctx->device);
    NMI_HIP_TRY(ctx, hipMemcpy(h_counts, s.d_counts.as<>(), (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
    return NMI_OK;
}

// The frame settings: later frame submissions read them at their upload; tickets already submitted are not affected.
int nmi_stream_set_distortion(nmi_stream *st, const double K[9], const float dist[5])
{
    return st ? intake_set_distortion(&st->intake, K, dist) : NMI_ERR_INVALID_ARGUMENT;
}

int nmi_stream_set_distortion_fisheye(nmi_stream *st, const double K[9], const double K_raw[9], const float dist[4])
{
    return st ? intake_set_distortion_fisheye(&st->intake, K, K_raw, dist) : NMI_ERR_INVALID_ARGUMENT;
}

int nmi_stream_set_frame_reduction(nmi_stream *st, int32_t factor, int32_t format, int64_t pitch)
{
    return st ? intake_set_frame(&st->intake, st->ctx->params.width, st->ctx->params.height, factor, format, pitch) : NMI_ERR_INVALID_ARGUMENT;
}

int nmi_stream_set_frame_format(nmi_stream *st, int32_t format, int64_t pitch) { return nmi_stream_set_frame_reduction(st, 1, format, pitch); }

int nmi_stream_set_tone_map(nmi_stream *st, const nmi_tone_map *tm)
{
    return st ? intake_set_tone_map(&st->intake, st->ctx->params.width, st->ctx->params.height, tm) : NMI_ERR_INVALID_ARGUMENT;
}

int nmi_stream_set_valid_range(nmi_stream *st, int32_t lo, int32_t hi)
{
    return st ? intake_set_valid_range(&st->intake, lo, hi) : NMI_ERR_INVALID_ARGUMENT;
}

int nmi_stream_keep_ratings(nmi_stream *st, int32_t enabled)
{
    if (!st) return NMI_ERR_INVALID_ARGUMENT;
    st->keep_ratings = enabled != 0;
    return NMI_OK;
}

int nmi_stream_copy_ratings(nmi_stream *st, int64_t ticket, float *h_ratings, int64_t n)
{
    if (!st || !h_ratings || ticket < 0 || ticket >= st->next_ticket) return NMI_ERR_INVALID_ARGUMENT;
    nmi_stream::Slot &s = st->slots[ticket % st->depth];
    // valid from nmi_stream_wait(ticket) until the slot is submitted to again
    if (s.ticket != ticket || !s.waited || s.failed || !s.d_ratings || n != (int64_t)s.S * s.Wn) return NMI_ERR_INVALID_ARGUMENT;
    nmi_ctx *ctx = st->ctx;
    DeviceGuard guard(ctx->device);
    NMI_HIP_TRY(ctx, hipMemcpy(h_ratings, s.d_ratings.as<>(), (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    return NMI_OK;
}

int nmi_stream_wait(nmi_stream *st, int64_t ticket, int64_t *h_best_index, float *h_best_score)
{
    if (!st || ticket < 0 || ticket >= st->next_ticket) return NMI_ERR_INVALID_ARGUMENT;
    nmi_stream::Slot &s = st->slots[ticket % st->depth];
    if (s.ticket != ticket || s.waited) return NMI_ERR_INVALID_ARGUMENT;  // overwritten or already collected
    nmi_ctx *ctx = st->ctx;
    DeviceGuard guard(ctx->device);
    NMI_HIP_TRY(ctx, hipEventSynchronize(s.done));
    s.waited = true;
    if (split_launch_failed(ctx, s.launch)) {
        // This ticket's search (a small grid on the split kernel) timed out in a hand-off.  Its render stack is still in the
        // slot; if its warp stack is too (no later frame has refilled that buffer) the search is redone here, behind
        // whatever was submitted since, by nmi_grid_kernel (the split forms are paused now).  Otherwise the ticket fails:
        // NMI_ERR_NOT_READY, its rating table is withheld, and the caller submits the level again.
        if (st->warp_gen[s.warp_buf] != s.warp_gen) {
            s.failed = true;
            ctx->detail = kSplitTimeoutTicketLost;
            return NMI_ERR_NOT_READY;
        }
        // (enqueue-only and unchecked: never a split form)
        SearchRequest rq = SearchRequest::block(s.d_renders.as<uint8_t>(), s.S, s.s_offset, s.S_total, st->d_warps[s.warp_buf].as<uint8_t>(), s.Wn,
                                                s.w_offset);
        rq.d_ratings = st->keep_ratings ? s.d_ratings.as<float>() : nullptr;
        rq.out_key = s.d_key.as<unsigned long long>();
        const int rc = enqueue_grid(ctx, rq, &s.launch);
        if (rc != NMI_OK) {
            s.failed = true;
            return rc;
        }
        NMI_HIP_TRY(ctx, hipMemcpyAsync(s.h_key.as<>(), s.d_key.as<>(), sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
        NMI_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        ctx->detail = kSplitTimeoutTicketNote;
    }
    return nmi_key_unpack(*s.h_key.as<unsigned long long>(), h_best_index, h_best_score);
}

}  // extern "C"
