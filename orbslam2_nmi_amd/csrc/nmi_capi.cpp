// nmi_capi.cpp -- the C ABI declared in include/nmi_hip.h on top of the gfx950 kernels: context, options, search.
//
// Host orchestration that replaces CUDAF::NMIWithCuda_noMask (Thirdparty/CUDA_Functions/kernel.cu:49-114)
// and the candidate loop + arg-max of Tracking::RelocalizeWithNMI (src/Tracking.cc:1879-1905,1952):
// a persistent context owns every buffer, one launch scores a whole candidate grid, and the only
// host<->device traffic per search is one 8-byte key.
#include <sched.h>

#include "nmi_ctx.h"

namespace nmi_internal {

int hip_fail(nmi_ctx *ctx, hipError_t e, const char *what)
{
    if (ctx) {
        char buf[256];
        snprintf(buf, sizeof buf, "%s: %s (%d)", what, hipGetErrorString(e), (int)e);
        ctx->detail = buf;
    }
    return NMI_ERR_HIP - (int)e;
}



// Visiting order of the candidates of an S x Wn grid in tiles (nmi_search_plan.h): the levels', streams', masked and covered searches'.
void build_order(int S, int Wn, int *order) { nmi::build_tile_order(S, Wn, order); }

// The cached visiting order for this grid shape (device pointer in *d_order), built and uploaded on first use.  grid > 0: the
// order that keeps one warp per workgroup of a launch of `grid` workgroups (build_search_order), which depends on the grid and is
// cached under it; grid = 0: the tiles.  Never
// synchronises the stream on a hit or on a miss with a free entry; only evicting the least recently used of kOrderCache
// shapes waits (its table may still be read by a kernel in flight).
int ensure_order(nmi_ctx *ctx, int S, int Wn, int grid, const int **d_order)
{
    *d_order = nullptr;
    if (!ctx->xcd_tiling) return NMI_OK;
    const int64_t total = (int64_t)S * Wn;
    nmi_ctx::OrderEntry *victim = nullptr;
    for (auto &e : ctx->orders) {
        if (e.S == S && e.Wn == Wn && e.grid == grid) {
            e.last_use = ++ctx->order_clock;
            *d_order = e.d.as<int>();
            return NMI_OK;
        }
        if (!victim || (!e.d && victim->d) || (!e.d == !victim->d && e.last_use < victim->last_use)) victim = &e;
    }
    nmi_ctx::OrderEntry &e = *victim;
    if (e.d) NMI_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // eviction: the old table / staging copy may be in use
    e.S = e.Wn = -1;
    const size_t bytes = (size_t)total * sizeof(int);
    NMI_HIP_TRY(ctx, e.d.grow(bytes));  // (waited above)
    NMI_HIP_TRY(ctx, e.h.grow(bytes, nmi_mem::kPinned));
    if (grid > 0) nmi::build_search_order(S, Wn, grid, e.h.as<int>());
    else build_order(S, Wn, e.h.as<int>());
    NMI_HIP_TRY(ctx, hipMemcpyAsync(e.d.as<int>(), e.h.as<int>(), bytes, hipMemcpyHostToDevice, ctx->stream));
    e.S = S;
    e.Wn = Wn;
    e.grid = grid;
    e.last_use = ++ctx->order_clock;
    *d_order = e.d.as<int>();
    return NMI_OK;
}

nmi::PlanInputs plan_inputs(const nmi_ctx *ctx, nmi::SearchForm form, int64_t total, const nmi::GridArgs &a)
{
    nmi::PlanInputs in;
    in.compute_units = ctx->compute_units;
    in.workgroups = ctx->workgroups;
    in.hist_variant = ctx->hist_variant;
    in.split_mode = ctx->split_mode;
    in.split_pixels = ctx->split_pixels;
    in.shift = ctx->shift;
    in.use_bg = ctx->params.use_bg != 0;
    in.phase_mask = ctx->phase_mask;
    in.content_path = ctx->content_path;
    in.xcd_tiling = ctx->xcd_tiling != 0;
    in.cooldown = ctx->split_cooldown > 0;
    in.few_hint = ctx->few_hint;
    in.total = total;
    in.width = a.width;
    in.npix = ctx->npix;
    in.vec_ok = a.vec_ok != 0;
    in.form = form;
    return in;
}

// the owner's share of a candidate's pixels: an equal one plus what it can add while its helpers' counters travel
double pix_owner_share(const nmi_ctx *ctx, int pix)
{
    const double owner_px = ((double)ctx->npix + (double)(pix - 1) * ctx->pix_owner_bias) / pix;
    return owner_px < ctx->npix ? owner_px / ctx->npix : 1.0;
}

static int ensure_pix_timeouts(nmi_ctx *ctx)
{
    NMI_HIP_TRY(ctx, ctx->d_pix_timeouts.grow(nmi::kPixHealWords * sizeof(uint32_t), ctx->stream, /*zero=*/true));
    return NMI_OK;
}

// Epoch of the next split launch.  Slab granules carry all 32 bits, block granules the low 16: neither may be 0 (the
// cleared state), and whenever the low 16 bits wrap the blocks are cleared so that no granule older than 65535 launches
// can show the current tag (the slabs likewise when all 32 bits wrap).
static int next_split_epoch(nmi_ctx *ctx, uint32_t *epoch)
{
    uint32_t e = ctx->split_epoch + 1;
    if ((e & 0xFFFFu) == 0) {
        if (ctx->d_blocks) NMI_HIP_TRY(ctx, hipMemsetAsync(ctx->d_blocks.as<>(), 0, ctx->d_blocks.size(), ctx->stream));
        if (ctx->d_pix_blocks) NMI_HIP_TRY(ctx, hipMemsetAsync(ctx->d_pix_blocks.as<>(), 0, ctx->d_pix_blocks.size(), ctx->stream));  // (its tags: 31 bits)
        if (e == 0 && ctx->d_slabs) NMI_HIP_TRY(ctx, hipMemsetAsync(ctx->d_slabs.as<>(), 0, ctx->d_slabs.size(), ctx->stream));
        ++e;
    }
    ctx->split_epoch = *epoch = e;
    return NMI_OK;
}

int prepare_pix_handoff(nmi_ctx *ctx, uint32_t *epoch)
{
    if (*epoch == 0) {
        const int rc = next_split_epoch(ctx, epoch);
        if (rc != NMI_OK) return rc;
    }
    return ensure_pix_timeouts(ctx);
}

// A hand-off buffer of at least `bytes`, zero when allocated (tag / epoch 0 = never written); growing waits for the stream.  The
// pixel-range kernels' blocks are a buffer of their own: the row-split kernel tags its granules with 16 bits in the top of an
// 8-byte word, which a packed counter of the other kernel's layout can equal.
static int ensure_zeroed(nmi_ctx *ctx, DeviceBuffer &buf, size_t bytes)
{
    NMI_HIP_TRY(ctx, buf.grow(bytes, ctx->stream, /*zero=*/true));
    return NMI_OK;
}

int prepare_search(nmi_ctx *ctx, const nmi::SearchPlan &plan, nmi::GridArgs &a)
{
    const int64_t total = (int64_t)a.S_local * a.Wn;
    int rc = NMI_OK;
    if (plan.kind == nmi::SearchKernel::split) {
        rc = ensure_zeroed(ctx, ctx->d_slabs, (size_t)(total > 128 ? total : 128) * sizeof(nmi::SplitSlab));
        if (rc == NMI_OK && plan.pix_parts > 1) rc = ensure_zeroed(ctx, ctx->d_blocks, (size_t)total * nmi::split_block_bytes_per_candidate(plan.pix_parts));
        if (rc == NMI_OK) rc = next_split_epoch(ctx, &a.epoch);
        a.slabs = ctx->d_slabs.as<nmi::SplitSlab>();
        a.blocks = ctx->d_blocks.as<unsigned long long>();
        a.split_error = ctx->split_error.device<uint32_t>();
    } else if (plan.kind == nmi::SearchKernel::pix) {
        rc = ensure_zeroed(ctx, ctx->d_pix_blocks, nmi::pix_block_bytes((int)total, plan.pix));
        if (rc == NMI_OK) rc = prepare_pix_handoff(ctx, &a.epoch);
        a.blocks = ctx->d_pix_blocks.as<unsigned long long>();
    } else if (plan.order_table) {
        rc = ensure_order(ctx, a.S_local, a.Wn, plan.shared_order ? plan.workgroups : 0, &a.order);
    }
    if (rc != NMI_OK) return rc;
#ifdef NMI_BUILD_ABLATIONS
    if (plan.scratch && plan.workgroups > ctx->scratch_workgroups) {
        ctx->scratch_workgroups = 0;
        const int alloc = plan.workgroups > ctx->compute_units ? plan.workgroups : ctx->compute_units;
        NMI_HIP_TRY(ctx, ctx->d_scratch.grow(nmi::grid_kernel_scratch_bytes(alloc), ctx->stream));
        ctx->scratch_workgroups = alloc;
        a.scratch = ctx->d_scratch.as<uint32_t>();
    }
#endif
    if (plan.probe) a.plan = ctx->d_plan.as<nmi::LevelPlan>();  // the search doubles as a probe (few-levels: the plan of its own probe)
    if (plan.kind == nmi::SearchKernel::few_levels) {
        const size_t need = (size_t)(a.S_local + a.Wn) * (size_t)ctx->npix;
        // with headroom: a coarse-to-fine search alternates between grid shapes, and growing drains the stream
        if (need > ctx->d_rank_stacks.size()) NMI_HIP_TRY(ctx, ctx->d_rank_stacks.grow(need + need / 2, ctx->stream));
    }
    return NMI_OK;
}

// Only launches whose winner the host will poll for post to the mailbox (one bit of sequence is enough because those calls
// are blocking, hence strictly alternating).  The sequence numbers, the key-slot flip, the "posted" flag and the launch
// record are committed here, once the launch has been accepted: a failed launch leaves the protocol in step.  An empty
// search (launched = false) keeps its key slot for the next launch: the slot is still "zero on entry".
int commit_launch(nmi_ctx *ctx, bool post, bool post_score, const SearchLaunch &rec, bool launched, SearchLaunch *out)
{
    if (post) ++ctx->seq;
    if (post_score) ++ctx->pair_seq;
    ctx->posted = post;
    ctx->last_slot = ctx->slot;
    ctx->last = rec;
    if (out) *out = rec;
    if (!launched) return NMI_OK;
    ctx->slot ^= 1;
    if (ctx->profiling) {
        NMI_HIP_TRY(ctx, hipEventRecord(ctx->ev_stop, ctx->stream));
        ctx->have_timing = true;
    }
    return NMI_OK;
}

// The grid arguments every search starts from: the request's block, the frame geometry, the key slots of this launch.
nmi::GridArgs grid_args(const nmi_ctx *ctx, const SearchRequest &rq, bool post, bool post_score)
{
    const nmi_params &p = ctx->params;
    nmi::GridArgs a{};
    a.render_stack = rq.render_stack;
    a.warp_stack = rq.warp_stack;
    a.S_local = rq.S_local;
    a.Wn = rq.Wn;
    a.s_offset = rq.s_offset;
    a.S_total = rq.S_total;
    a.w_offset = rq.w_offset;
    nmi::set_geometry(a, p.width, p.height, rq.render_stack, rq.warp_stack, p.render_bottom_up != 0);
    a.shift = ctx->shift;
    a.mode = p.mode;
    a.ratings = rq.d_ratings;
    a.key = ctx->d_keys.as<unsigned long long>() + ctx->slot;
    a.reset_key = ctx->d_keys.as<unsigned long long>() + (ctx->slot ^ 1);
    a.out_key = rq.out_key;
    a.done = ctx->d_done.as<unsigned int>();
    a.mailbox = post ? ctx->mailbox.as<nmi::Mailbox>() : nullptr;
    a.score_post = post_score ? ctx->score_mailbox.as<unsigned long long>() : nullptr;
    a.seq = post ? ctx->seq + 1 : (post_score ? ctx->pair_seq + 1 : 0);
    a.hist_variant = ctx->hist_variant;
    return a;
}

// Five steps: the arguments, the plan, its resources, the launch the plan names, the record.
int enqueue_grid(nmi_ctx *ctx, const SearchRequest &rq, SearchLaunch *launched)
{
    const nmi_params &p = ctx->params;
    const bool post = rq.post && ctx->result_path == 1, post_score = rq.post_score && ctx->result_path == 1;
    nmi::GridArgs a = grid_args(ctx, rq, post, post_score);
    if (rq.pair_renders) {  // nmi_eval_pairs: per-pair pointers; the 16-byte path needs every one of them aligned
        a.pair_renders = rq.pair_renders;
        a.pair_warps = rq.pair_warps;
        uintptr_t bits = 0;
        for (int i = 0; i < rq.S_local; ++i) bits |= (uintptr_t)rq.pair_renders_host[i] | (uintptr_t)rq.pair_warps_host[i];
        if (bits % 16) nmi::set_geometry(a, p.width, p.height, (const void *)1, (const void *)1, p.render_bottom_up != 0);
    }
    a.table = ctx->table.as<float>();
    a.scratch = ctx->d_scratch.as<uint32_t>();
    a.dbg_joint = rq.dbg_joint;
    a.dbg_h1 = rq.dbg_h1;
    a.dbg_h2 = rq.dbg_h2;
    a.dbg_sums = rq.dbg_sums;
    a.dbg_stamps = ctx->dbg_stamps;

    const int64_t total = (int64_t)rq.S_local * rq.Wn;
    if (total == 0) {
        // nothing to score: the winner is "none" (key 0); publish it the way the kernel would.  The key slot keeps its
        // "zero on entry" state for the next launch (nothing ever writes a winner into a ping-pong slot from outside:
        // the RCCL form reduces into ctx->d_reduced_key).
        if (rq.out_key) NMI_HIP_TRY(ctx, hipMemsetAsync(rq.out_key, 0, sizeof(unsigned long long), ctx->stream));
        NMI_HIP_TRY(ctx, hipMemsetAsync(ctx->d_keys.as<unsigned long long>() + ctx->slot, 0, sizeof(unsigned long long), ctx->stream));
        NMI_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        if (post) ctx->mailbox.as<nmi::Mailbox>()->word = (unsigned long long)((ctx->seq + 1) & 1u) << 63;
        return commit_launch(ctx, post, false, SearchLaunch{}, /*launched=*/false, launched);
    }
    nmi::PlanInputs in = plan_inputs(ctx, nmi::SearchForm::plain, total, a);
    in.debug_exports = rq.dbg_joint || rq.dbg_h1 || rq.dbg_h2 || rq.dbg_sums;
    in.stamps = ctx->dbg_stamps != nullptr;
    in.pair_pointers = rq.pair_renders != nullptr;
    // does somebody look for a split-kernel timeout after this launch?  (blocking calls, nmi_eval_pairs, stream tickets, RCCL form)
    in.split_checked = rq.post || rq.post_score || rq.caller_checks_split || in.pair_pointers;
    // What the most recent search found in its stacks (nr, nw), posted by the device: by the probe that goes with every
    // few-levels launch, or by nmi_grid_kernel itself -- every general search counts the bins of its candidates'
    // marginals on the way (publish_seen / post_seen), so a change of content shows after ONE search, with no extra launch.
    const unsigned long long posted = __atomic_load_n(ctx->level_post.as<unsigned long long>(), __ATOMIC_ACQUIRE);
    if ((uint32_t)(posted >> 32) != ctx->level_seen) {
        const uint32_t joint = (uint32_t)((posted >> 16) & 0xFFFFu) * (uint32_t)(posted & 0xFFFFu);
        in.few_hint = joint > 0 && joint <= (uint32_t)ctx->fewlevels_bins;
    }
    const nmi::SearchPlan plan = nmi::plan_search(in);
    // the two stateful steps of the decision: a held-back split form takes one unit off the pause, a consulted hint is kept
    if (plan.used_cooldown) --ctx->split_cooldown;
    if (plan.read_hint) {
        ctx->level_seen = (uint32_t)(posted >> 32);
        ctx->few_hint = in.few_hint;
    }
    if (plan.unsupported) return NMI_ERR_UNSUPPORTED;  // (nmi_eval_pairs decides first)
    a.phase_mask = plan.phase_mask;
    const int rc = prepare_search(ctx, plan, a);
    if (rc != NMI_OK) return rc;

    const bool use_bg = p.use_bg != 0;
    if (ctx->profiling) NMI_HIP_TRY(ctx, hipEventRecord(ctx->ev_start, ctx->stream));
    switch (plan.kind) {
    case nmi::SearchKernel::split:
        NMI_HIP_TRY(ctx, nmi::launch_split(a, plan.parts, plan.pix_parts, plan.workgroups, use_bg, ctx->stream));
        break;
    case nmi::SearchKernel::pix:
        NMI_HIP_TRY(ctx, nmi::launch_pix(a, plan.pix, pix_owner_share(ctx, plan.pix), use_bg, nullptr, ctx->d_pix_timeouts.as<uint32_t>(), ctx->stream));
        break;
    case nmi::SearchKernel::few_levels:
        NMI_HIP_TRY(ctx, nmi::launch_levels(rq.render_stack, rq.S_local, rq.warp_stack, rq.Wn, ctx->npix, ctx->shift, ctx->d_plan.as<nmi::LevelPlan>(),
                                            ctx->level_post.as<unsigned long long>(), ++ctx->level_seq, (uint32_t)ctx->fewlevels_bins, true, ctx->stream));
        NMI_HIP_TRY(ctx, nmi::launch_fewlevels(a, ctx->d_rank_stacks.as<uint8_t>(), ctx->d_rank_stacks.as<uint8_t>() + (size_t)rq.S_local * ctx->npix,
                                               plan.workgroups, use_bg, ctx->stream));
        NMI_HIP_TRY(ctx, nmi::launch_grid_gated(a, plan.workgroups, use_bg, ctx->stream));
        break;
    default:
        NMI_HIP_TRY(ctx, nmi::launch_grid(a, plan.workgroups, use_bg, ctx->stream));
    }
    const bool few = plan.kind == nmi::SearchKernel::few_levels;
    return commit_launch(ctx, post, post_score, SearchLaunch{plan.kind, plan.parts, plan.pix, plan.parts ? a.epoch : 0, few ? 1 : 0},
                         /*launched=*/true, launched);
}

// A hand-off of the split kernel timed out (its workgroups could not all run at once -- e.g. the device exposes fewer
// compute units to this process than it reports): wait for the launch to drain, switch the split forms off for this
// context and tell the caller to redo the call, which then goes through nmi_grid_kernel.
bool split_launch_failed(nmi_ctx *ctx, const SearchLaunch &launch)
{
    if (!launch.parts) return false;
    const uint32_t epoch = launch.epoch;
    uint32_t *word = ctx->split_error.as<uint32_t>() + (epoch % nmi::kSplitRing);
    if (__atomic_load_n(word, __ATOMIC_ACQUIRE) != epoch) {
        // a split launch that went through re-arms the short cooldown -- if it was issued AFTER the last pause was set: a sibling
        // of the failed launch (same nmi_eval_pairs batch, stream tickets already in flight) says nothing about the retry
        if ((int32_t)(epoch - ctx->split_cooldown_epoch) > 0) ctx->split_backoff = nmi_ctx::kSplitBackoffMin;
        return false;
    }
    (void)hipStreamSynchronize(ctx->stream);
    __atomic_store_n(word, 0u, __ATOMIC_RELEASE);
    ++ctx->split_timeouts;
    ctx->split_cooldown = ctx->split_backoff;
    ctx->split_cooldown_epoch = ctx->split_epoch;
    if (ctx->split_backoff < nmi_ctx::kSplitBackoffMax) ctx->split_backoff *= 2;
    return true;
}

// Call once the most recent launch's result has arrived (the kernel raises the flag before it posts anything).
bool split_timed_out(nmi_ctx *ctx) { return split_launch_failed(ctx, ctx->last); }

const char *const kSplitTimeoutNote = "split kernel hand-off timed out; call redone by the one-workgroup kernel, split forms paused (nmi_split_status)";
const char *const kSplitTimeoutTicketNote = "split kernel hand-off timed out; ticket redone by the one-workgroup kernel, split forms paused (nmi_split_status)";
const char *const kSplitTimeoutTicketLost = "split kernel hand-off timed out and the ticket's warp stack is gone: submit the level again";

// Polls a pinned host word until (word & mask) == want; *out receives the word.  NMI_OPT_WAIT_MODE 0 spins (lowest
// latency; occupies the calling core for the duration of the search), 1 yields the core between polls (the Tracking
// thread shares the host with LocalMapping / LoopClosing).  A faulted or drained stream ends the wait: returns
// NMI_ERR_NOT_READY when the stream is idle and the word still does not match.
int wait_word(nmi_ctx *ctx, const volatile unsigned long long *word, unsigned long long mask, unsigned long long want,
              unsigned long long *out)
{
    const uint64_t check_every = ctx->wait_mode == 1 ? 0x3F : 0xFFFF;
    for (uint64_t spin = 0;; ++spin) {
        const unsigned long long v = __atomic_load_n(word, __ATOMIC_ACQUIRE);
        if ((v & mask) == want) {
            *out = v;
            return NMI_OK;
        }
        if (ctx->wait_mode == 1) sched_yield();
        if ((spin & check_every) == check_every) {
            const hipError_t q = hipStreamQuery(ctx->stream);
            if (q == hipSuccess) {
                const unsigned long long v2 = __atomic_load_n(word, __ATOMIC_ACQUIRE);
                *out = v2;
                return (v2 & mask) == want ? NMI_OK : NMI_ERR_NOT_READY;
            }
            if (q != hipErrorNotReady) return hip_fail(ctx, q, "hipStreamQuery");
        }
    }
}

// Blocks until the launch numbered ctx->seq has published its winner and returns it.
int fetch_key(nmi_ctx *ctx, unsigned long long *key)
{
    if (ctx->posted) {
        // The last workgroup stores (key | parity << 63) to fine-grained pinned memory; poll that one word.
        unsigned long long word = 0;
        const int rc = wait_word(ctx, &ctx->mailbox.as<nmi::Mailbox>()->word, 1ull << 63, (unsigned long long)(ctx->seq & 1u) << 63, &word);
        if (rc == NMI_OK) {
            *key = word & 0x7FFFFFFFFFFFFFFFull;
            return NMI_OK;
        }
        if (rc != NMI_ERR_NOT_READY) return rc;  // stream drained without a post: fall through to the copy path
    }
    NMI_HIP_TRY(ctx, hipMemcpyAsync(ctx->h_key.as<>(), ctx->d_keys.as<unsigned long long>() + ctx->last_slot, sizeof(unsigned long long),
                                    hipMemcpyDeviceToHost, ctx->stream));
    NMI_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    *key = *ctx->h_key.as<unsigned long long>();
    return NMI_OK;
}

// Uploads `n` floats through a slot of the ring on the context's stream; *d_out is the device copy (valid for work
// enqueued on that stream until the slot comes round again).
int stage_floats(nmi_ctx *ctx, nmi_mem::UploadRing &ring, const float *h_src, size_t n, float **d_out)
{
    nmi_mem::UploadRing::Slot slot;
    NMI_HIP_TRY(ctx, ring.acquire(n, ctx->stream, &slot));
    memcpy(slot.h, h_src, n * sizeof(float));
    NMI_HIP_TRY(ctx, ring.upload(slot, ctx->stream));
    NMI_HIP_TRY(ctx, ring.release(slot, ctx->stream));
    *d_out = slot.d;
    return NMI_OK;
}

int check_grid_args(nmi_ctx *ctx, const uint8_t *render_stack, int S_local, int s_offset, int S_total,
                    const uint8_t *warp_stack, int Wn)
{
    if (!ctx) return NMI_ERR_INVALID_ARGUMENT;
    ctx->detail.clear();
    if (S_local < 0 || Wn < 0 || s_offset < 0 || S_total < S_local || s_offset + S_local > S_total)
        return NMI_ERR_INVALID_ARGUMENT;
    if ((S_local > 0 && !render_stack) || (Wn > 0 && !warp_stack)) return NMI_ERR_INVALID_ARGUMENT;
    if ((int64_t)S_total * Wn >= 0x7FFFFFFFll) return NMI_ERR_UNSUPPORTED;  // index lives in 32 bits of the key
    return NMI_OK;
}

}  // namespace nmi_internal

using namespace nmi_internal;

extern "C" {

int nmi_abi_version(void) { return NMI_HIP_ABI_VERSION; }

const char *nmi_error_string(int code)
{
    if (code == NMI_OK) return "ok";
    if (code == NMI_ERR_INVALID_ARGUMENT) return "invalid argument";
    if (code == NMI_ERR_UNSUPPORTED) return "unsupported configuration";
    if (code == NMI_ERR_NO_DEVICE) return "no usable HIP device";
    if (code == NMI_ERR_NOT_READY) return "not ready";
    if (code <= NMI_ERR_RCCL) return "RCCL error";
    if (code <= NMI_ERR_HIP) return hipGetErrorString((hipError_t)(NMI_ERR_HIP - code));
    return "unknown error";
}

const char *nmi_last_error_detail(nmi_ctx *ctx) { return ctx ? ctx->detail.c_str() : ""; }

int nmi_params_default(nmi_params *p, int32_t width, int32_t height)
{
    if (!p) return NMI_ERR_INVALID_ARGUMENT;
    memset(p, 0, sizeof *p);
    p->width = width;
    p->height = height;
    p->bins = 256;             // HISTOGRAM256_BIN_COUNT, NMI.cuh:39
    p->mode = NMI_MODE_SUC;    // kernel.cuh:22-23 + NMI.cu:344,352
    p->use_bg = 1;             // nmi_prop_BG true, allProperties.hpp:38
    p->render_bottom_up = 1;   // NMI.cu:82
    p->device = -1;
    p->max_candidates = 0;
    p->stream = nullptr;
    return NMI_OK;
}

int nmi_create(const nmi_params *params, nmi_ctx **out_ctx)
{
    if (!params || !out_ctx) return NMI_ERR_INVALID_ARGUMENT;
    *out_ctx = nullptr;
    const nmi_params &p = *params;
    if (p.width <= 0 || p.height <= 0) return NMI_ERR_INVALID_ARGUMENT;
    if ((int64_t)p.width * p.height > (1ll << 24)) return NMI_ERR_UNSUPPORTED;  // counts must stay exact in fp32
    if (p.mode != NMI_MODE_SUC && p.mode != NMI_MODE_ENMI) return NMI_ERR_INVALID_ARGUMENT;
    int shift = -1;
    for (int k = 0; k <= 4; ++k)
        if (p.bins == (256 >> k)) shift = k;
    if (shift < 0) return NMI_ERR_UNSUPPORTED;
    for (int r : p.reserved)
        if (r != 0) return NMI_ERR_INVALID_ARGUMENT;

    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return NMI_ERR_NO_DEVICE;
    int dev = p.device;
    if (dev < 0 && hipGetDevice(&dev) != hipSuccess) return NMI_ERR_NO_DEVICE;
    if (dev >= ndev) return NMI_ERR_INVALID_ARGUMENT;

    nmi_ctx *ctx = new (std::nothrow) nmi_ctx;
    if (!ctx) return NMI_ERR_INVALID_ARGUMENT;
    ctx->params = p;
    ctx->device = dev;
    ctx->npix = p.width * p.height;
    ctx->shift = shift;
    DeviceGuard guard(dev);

    hipDeviceProp_t prop;
    const char *what = "hipGetDeviceProperties";  // the step in hand: named by the detail text if it fails
    hipError_t e = hipGetDeviceProperties(&prop, dev);
    if (e == hipSuccess && (size_t)nmi::grid_kernel_lds_bytes() > prop.sharedMemPerBlock) {
        // The kernel keeps a whole packed joint histogram in LDS: it needs a CU with >= 136 KiB (gfx950: 160 KiB).
        delete ctx;
        return NMI_ERR_UNSUPPORTED;
    }
    if (e == hipSuccess) ctx->compute_units = prop.multiProcessorCount;
    auto step = [&](const char *name, auto &&call) {
        if (e == hipSuccess) what = name, e = call();
        return e == hipSuccess;
    };
    using nmi_mem::kPosted;
    constexpr size_t kWord = sizeof(unsigned long long);
    if (step("hipStreamCreateWithFlags", [&] { return ctx->own_stream.create(hipStreamNonBlocking); }))
        ctx->stream = p.stream ? (hipStream_t)p.stream : (hipStream_t)ctx->own_stream;
    hipStream_t st = ctx->stream;
    step("device buffer (table)", [&] { return ctx->table.alloc(((size_t)ctx->npix + 1) * sizeof(float)); });
    step("device buffer (key)", [&] { return ctx->d_keys.alloc(2 * kWord); });
    step("device buffer (done)", [&] { return ctx->d_done.alloc(sizeof(unsigned int)); });
    // on the context's own (non-blocking) stream: a legacy-stream hipMemset is not ordered against it
    step("hipMemsetAsync(key)", [&] { return hipMemsetAsync(ctx->d_keys.as<>(), 0, 2 * kWord, st); });
    step("hipMemsetAsync(done)", [&] { return hipMemsetAsync(ctx->d_done.as<>(), 0, sizeof(unsigned int), st); });
    if (step("pinned buffer (mailbox)", [&] { return ctx->mailbox.alloc(sizeof(nmi::Mailbox), kPosted); })) memset(ctx->mailbox.as<>(), 0, sizeof(nmi::Mailbox));
    step("device buffer (rating)", [&] { return ctx->d_pair_rating.alloc(sizeof(float)); });
    step("device buffer (reduced key)", [&] { return ctx->d_reduced_key.alloc(kWord); });
    if (step("pinned buffer (score mailbox)", [&] { return ctx->score_mailbox.alloc(2 * kWord, kPosted); })) memset(ctx->score_mailbox.as<>(), 0, 2 * kWord);
    if (step("pinned buffer (split error)", [&] { return ctx->split_error.alloc(nmi::kSplitRing * sizeof(uint32_t), kPosted); }))
        memset(ctx->split_error.as<>(), 0, nmi::kSplitRing * sizeof(uint32_t));
    step("pinned buffer (key)", [&] { return ctx->h_key.alloc(kWord, nmi_mem::kPinned); });
    if (step("pinned buffer (level post)", [&] { return ctx->level_post.alloc(64, kPosted); })) *ctx->level_post.as<unsigned long long>() = 0;
    step("device buffer (level plan)", [&] { return ctx->d_plan.alloc(sizeof(nmi::LevelPlan)); });
    step("hipMemsetAsync(level plan)", [&] { return hipMemsetAsync(ctx->d_plan.as<>(), 0, sizeof(nmi::LevelPlan), st); });
    // where the general kernel's last workgroup posts what its search found (every search is a content probe)
    nmi::LevelPlan *d_plan = ctx->d_plan.as<nmi::LevelPlan>();
    unsigned long long *d_post = ctx->level_post.device<unsigned long long>();
    const uint32_t max_joint = (uint32_t)ctx->fewlevels_bins;
    step("hipMemcpyAsync(level post)", [&] { return hipMemcpyAsync(&d_plan->seen_post, &d_post, sizeof d_post, hipMemcpyHostToDevice, st); });
    step("hipMemcpyAsync(level plan)", [&] { return hipMemcpyAsync(&d_plan->seen_max_joint, &max_joint, sizeof max_joint, hipMemcpyHostToDevice, st); });
    step("hipStreamSynchronize", [&] { return hipStreamSynchronize(st); });  // (d_post and max_joint are locals)
    step("hipEventCreate", [&] { return ctx->ev_start.create(hipEventDefault); });
    step("hipEventCreate", [&] { return ctx->ev_stop.create(hipEventDefault); });
    step("launch_table", [&] { return nmi::launch_table(ctx->table.as<float>(), ctx->npix, st); });
    step("hipStreamSynchronize", [&] { return hipStreamSynchronize(st); });
    if (e != hipSuccess) {
        const int rc = hip_fail(ctx, e, what);
        fprintf(stderr, "nmi_create: %s\n", ctx->detail.c_str());
        nmi_destroy(ctx);
        return rc;
    }
    *out_ctx = ctx;
    return NMI_OK;
}

int nmi_destroy(nmi_ctx *ctx)
{
    if (!ctx) return NMI_OK;
    DeviceGuard guard(ctx->device);
    if (ctx->own_stream) (void)hipStreamSynchronize(ctx->own_stream);
    delete ctx;
    return NMI_OK;
}

int nmi_set_stream(nmi_ctx *ctx, void *stream)
{
    if (!ctx) return NMI_ERR_INVALID_ARGUMENT;
    ctx->stream = stream ? (hipStream_t)stream : (hipStream_t)ctx->own_stream;
    return NMI_OK;
}

int nmi_synchronize(nmi_ctx *ctx)
{
    if (!ctx) return NMI_ERR_INVALID_ARGUMENT;
    DeviceGuard guard(ctx->device);
    NMI_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return NMI_OK;
}

int nmi_set_option(nmi_ctx *ctx, int32_t option, int64_t value)
{
    if (!ctx) return NMI_ERR_INVALID_ARGUMENT;
    switch (option) {
    case NMI_OPT_HIST_VARIANT:
        if (value < 0 || value > 4) return NMI_ERR_INVALID_ARGUMENT;
        if (value != 1 && value != 3 && !nmi::ablation_variants_built()) return NMI_ERR_UNSUPPORTED;  // -DNMI_BUILD_ABLATIONS
        ctx->hist_variant = (int)value;
        return NMI_OK;
    case NMI_OPT_SPLIT:
        if (value != -1 && value != 0 && value != 1 && value != 2 && value != 4 && value != 8) return NMI_ERR_INVALID_ARGUMENT;
        ctx->split_mode = (int)value;
        return NMI_OK;
    case NMI_OPT_SPLIT_PIXELS:
        if (value != -1 && (value < 1 || value > 8)) return NMI_ERR_INVALID_ARGUMENT;  // 3, 5 ... 8: with NMI_OPT_SPLIT 1 only
        ctx->split_pixels = (int)value;
        return NMI_OK;
    case NMI_OPT_PIX_OWNER_BIAS:
        if (value < 0 || value > (1 << 24)) return NMI_ERR_INVALID_ARGUMENT;
        ctx->pix_owner_bias = (int)value;
        return NMI_OK;
    case NMI_OPT_STAMPS:
        ctx->dbg_stamps = (unsigned long long *)(uintptr_t)value;
        return NMI_OK;
    case NMI_OPT_STAMP_CANDIDATE:
    case NMI_OPT_WAVE_SHARES:
        if (option == NMI_OPT_STAMP_CANDIDATE ? (value < 0 || value > 65535) : value == 0) return NMI_ERR_INVALID_ARGUMENT;
        {
            DeviceGuard guard(ctx->device);
            NMI_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            if (option == NMI_OPT_STAMP_CANDIDATE) ctx->stamp_candidate = (int)value;
            NMI_HIP_TRY(ctx, nmi::set_stamped_experiment(ctx->stamp_candidate, option == NMI_OPT_WAVE_SHARES ? (const uint32_t *)(uintptr_t)value : nullptr));
        }
        return NMI_OK;
    case NMI_OPT_WAIT_MODE:
        if (value < 0 || value > 1) return NMI_ERR_INVALID_ARGUMENT;
        ctx->wait_mode = (int)value;
        return NMI_OK;
    case NMI_OPT_PHASE_MASK:
        if (value < 0 || value > 1023) return NMI_ERR_INVALID_ARGUMENT;
        ctx->phase_mask = (int)value;
        return NMI_OK;
    case NMI_OPT_XCD_TILING:
        if (value < 0 || value > 1) return NMI_ERR_INVALID_ARGUMENT;
        ctx->xcd_tiling = (int)value;
        return NMI_OK;
    case NMI_OPT_RESULT_PATH:
        if (value < 0 || value > 1) return NMI_ERR_INVALID_ARGUMENT;
        ctx->result_path = (int)value;
        return NMI_OK;
    case NMI_OPT_TILE_QUEUE:
        if (value < 0 || value > (4ll << 20)) return NMI_ERR_INVALID_ARGUMENT;
        ctx->tile_queue_limit = (unsigned long long)value;
        return NMI_OK;
    case NMI_OPT_CLIP_QUEUE:
        if (value < 0) return NMI_ERR_INVALID_ARGUMENT;
        ctx->clip_queue_limit = (unsigned long long)value;
        return NMI_OK;
    case NMI_OPT_CONTENT_PATH:
        if (value < -1 || value > 1) return NMI_ERR_INVALID_ARGUMENT;
        ctx->content_path = (int)value;
        ctx->few_hint = false;
        {   // the device posts changes of its verdict only: start it from "not few" as well (blocking: a local is copied)
            DeviceGuard guard(ctx->device);
            const uint32_t zero = 0;
            NMI_HIP_TRY(ctx, hipMemcpyAsync(&ctx->d_plan.as<nmi::LevelPlan>()->seen_state, &zero, sizeof zero, hipMemcpyHostToDevice, ctx->stream));
            NMI_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        }
        return NMI_OK;
    case NMI_OPT_FEWLEVELS_BINS:
        if (value < 1 || value > nmi::fewlevels_max_joint()) return NMI_ERR_INVALID_ARGUMENT;
        ctx->fewlevels_bins = (int)value;
        {
            DeviceGuard guard(ctx->device);
            const uint32_t max_joint = (uint32_t)value, zero = 0;
            NMI_HIP_TRY(ctx, hipMemcpyAsync(&ctx->d_plan.as<nmi::LevelPlan>()->seen_max_joint, &max_joint, sizeof max_joint, hipMemcpyHostToDevice, ctx->stream));
            NMI_HIP_TRY(ctx, hipMemcpyAsync(&ctx->d_plan.as<nmi::LevelPlan>()->seen_state, &zero, sizeof zero, hipMemcpyHostToDevice, ctx->stream));
            NMI_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            ctx->few_hint = false;
        }
        return NMI_OK;
    case NMI_OPT_WORKGROUPS:
        if (value < 0 || value > (1 << 20)) return NMI_ERR_INVALID_ARGUMENT;
        ctx->workgroups = (int)value;
        return NMI_OK;
    default:
        return NMI_ERR_INVALID_ARGUMENT;
    }
}

int nmi_set_profiling(nmi_ctx *ctx, int32_t enabled)
{
    if (!ctx) return NMI_ERR_INVALID_ARGUMENT;
    ctx->profiling = enabled != 0;
    ctx->have_timing = false;
    return NMI_OK;
}

int nmi_last_kernel_ms(nmi_ctx *ctx, float *h_ms)
{
    if (!ctx || !h_ms) return NMI_ERR_INVALID_ARGUMENT;
    if (!ctx->have_timing) return NMI_ERR_NOT_READY;
    DeviceGuard guard(ctx->device);
    NMI_HIP_TRY(ctx, hipEventSynchronize(ctx->ev_stop));
    NMI_HIP_TRY(ctx, hipEventElapsedTime(h_ms, ctx->ev_start, ctx->ev_stop));
    return NMI_OK;
}

int nmi_get_info(nmi_ctx *ctx, int32_t *compute_units, int32_t *workgroups_per_launch, int32_t *lds_bytes)
{
    if (!ctx) return NMI_ERR_INVALID_ARGUMENT;
    if (compute_units) *compute_units = ctx->compute_units;
    if (workgroups_per_launch) *workgroups_per_launch = ctx->workgroups > 0 ? ctx->workgroups : ctx->compute_units;
    if (lds_bytes) *lds_bytes = nmi::grid_kernel_lds_bytes();
    return NMI_OK;
}

int nmi_last_content(nmi_ctx *ctx, int32_t *few_levels, int32_t *nr, int32_t *nw)
{
    if (!ctx) return NMI_ERR_INVALID_ARGUMENT;
    DeviceGuard guard(ctx->device);
    NMI_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    const unsigned long long posted = __atomic_load_n(ctx->level_post.as<unsigned long long>(), __ATOMIC_ACQUIRE);
    const int32_t r = (int32_t)((posted >> 16) & 0xFFFFu), w = (int32_t)(posted & 0xFFFFu);
    if (nr) *nr = r;
    if (nw) *nw = w;
    // a few-levels launch carries its own probe, so the post is about that very search -- and the probe's verdict
    // (LevelPlan::use, untouched since: the stream is idle) is what let one of the two scoring kernels behind it run.  Read it,
    // do not restate it: a restatement on the host agrees with any device-side slip at the limit.
    uint32_t use = 0;
    if (few_levels && ctx->last.few) {
        NMI_HIP_TRY(ctx, hipMemcpyAsync(&use, &ctx->d_plan.as<nmi::LevelPlan>()->use, sizeof use, hipMemcpyDeviceToHost, ctx->stream));
        NMI_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    if (few_levels) *few_levels = use ? 1 : 0;
    return NMI_OK;
}

int nmi_copy_term_table(nmi_ctx *ctx, float *h_out, int64_t n)
{
    if (!ctx || !h_out || n != (int64_t)ctx->npix + 1) return NMI_ERR_INVALID_ARGUMENT;
    DeviceGuard guard(ctx->device);
    NMI_HIP_TRY(ctx, hipMemcpyAsync(h_out, ctx->table.as<>(), (size_t)n * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    NMI_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return NMI_OK;
}

uint64_t nmi_key_pack(float score, int64_t global_linear_index)
{
    if (!(score >= 0.0f) || global_linear_index < 0 || global_linear_index >= 0xFFFFFFFFll) return 0;
    uint32_t bits = 0;
    if (score != 0.0f) memcpy(&bits, &score, sizeof bits);
    return ((uint64_t)bits << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)global_linear_index);
}

int nmi_key_unpack(uint64_t key, int64_t *global_linear_index, float *score)
{
    if (key == 0) {
        if (global_linear_index) *global_linear_index = -1;
        if (score) *score = 0.0f;
        return NMI_OK;
    }
    const uint32_t bits = (uint32_t)(key >> 32);
    if (global_linear_index) *global_linear_index = (int64_t)(0xFFFFFFFFu - (uint32_t)(key & 0xFFFFFFFFu));
    if (score) memcpy(score, &bits, sizeof bits);
    return NMI_OK;
}

int nmi_search_grid_shard(nmi_ctx *ctx, const uint8_t *render_stack, int32_t S_local, int32_t s_offset, int32_t S_total,
                          const uint8_t *warp_stack, int32_t Wn, float *d_ratings, uint64_t *d_key, uint64_t *h_key)
{
    return nmi_search_grid_block(ctx, render_stack, S_local, s_offset, S_total, warp_stack, Wn, 0, Wn, d_ratings, d_key, h_key);
}

int nmi_search_grid_block(nmi_ctx *ctx, const uint8_t *render_stack, int32_t S_local, int32_t s_offset, int32_t S_total,
                          const uint8_t *warp_stack, int32_t Wn_local, int32_t w_offset, int32_t Wn_total, float *d_ratings,
                          uint64_t *d_key, uint64_t *h_key)
{
    return search_block(ctx, render_stack, S_local, s_offset, S_total, warp_stack, Wn_local, w_offset, Wn_total, d_ratings, d_key, h_key,
                        /*caller_checks=*/false);
}

}  // extern "C"

int nmi_internal::search_block(nmi_ctx *ctx, const uint8_t *render_stack, int32_t S_local, int32_t s_offset, int32_t S_total,
                               const uint8_t *warp_stack, int32_t Wn_local, int32_t w_offset, int32_t Wn_total, float *d_ratings,
                               uint64_t *d_key, uint64_t *h_key, bool caller_checks)
{
    int rc = check_grid_args(ctx, render_stack, S_local, s_offset, S_total, warp_stack, Wn_local);
    if (rc != NMI_OK) return rc;
    if (w_offset < 0 || Wn_total < Wn_local || w_offset + Wn_local > Wn_total) return NMI_ERR_INVALID_ARGUMENT;
    if ((int64_t)S_total * Wn_total >= 0x7FFFFFFFll) return NMI_ERR_UNSUPPORTED;  // index lives in 32 bits of the key
    const int32_t Wn = Wn_local;
    DeviceGuard guard(ctx->device);
    SearchRequest rq = SearchRequest::block(render_stack, S_local, s_offset, S_total, warp_stack, Wn, w_offset);
    rq.d_ratings = d_ratings;
    rq.out_key = (unsigned long long *)d_key;
    rq.post = h_key != nullptr;
    rq.caller_checks_split = caller_checks;
    rc = enqueue_grid(ctx, rq);
    if (rc != NMI_OK) return rc;
    if (h_key) {
        unsigned long long k = 0;
        rc = fetch_key(ctx, &k);
        if (rc != NMI_OK) return rc;
        if (split_timed_out(ctx)) {  // (the cooldown now routes the redo through nmi_grid_kernel)
            rc = search_block(ctx, render_stack, S_local, s_offset, S_total, warp_stack, Wn_local, w_offset, Wn_total, d_ratings, d_key,
                              h_key, false);
            if (rc == NMI_OK) ctx->detail = kSplitTimeoutNote;
            return rc;
        }
        *h_key = k;
        // The winner is posted by the last workgroup before the kernel has retired: a caller that asked for the rating
        // table may read it right after this call, from any stream, so the table must be complete (and written back).
        if (d_ratings || d_key) NMI_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    return NMI_OK;
}

extern "C" {

int nmi_split_status(nmi_ctx *ctx, int32_t *timeouts, int32_t *cooldown_calls_left, int32_t *next_cooldown, int32_t *last_launch_parts)
{
    if (!ctx) return NMI_ERR_INVALID_ARGUMENT;
    if (timeouts) *timeouts = (int32_t)ctx->split_timeouts;
    if (cooldown_calls_left) *cooldown_calls_left = (int32_t)ctx->split_cooldown;
    if (next_cooldown) *next_cooldown = (int32_t)ctx->split_backoff;
    if (last_launch_parts) *last_launch_parts = ctx->last.parts;
    return NMI_OK;
}

// the pixel-range kernels' heal counters so far (kPixHeal*; zeros before the first such launch); waits for the stream
static int read_pix_heal(nmi_ctx *ctx, uint32_t (&n)[nmi::kPixHealWords])
{
    for (uint32_t &x : n) x = 0;
    if (!ctx->d_pix_timeouts) return NMI_OK;
    DeviceGuard guard(ctx->device);
    NMI_HIP_TRY(ctx, hipMemcpyAsync(n, ctx->d_pix_timeouts.as<>(), sizeof n, hipMemcpyDeviceToHost, ctx->stream));
    NMI_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return NMI_OK;
}

int nmi_pix_status(nmi_ctx *ctx, int32_t *last_launch_ranges, int32_t *healed)
{
    if (!ctx) return NMI_ERR_INVALID_ARGUMENT;
    if (last_launch_ranges) *last_launch_ranges = ctx->last.pix;
    if (healed) {
        uint32_t n[nmi::kPixHealWords];
        const int rc = read_pix_heal(ctx, n);
        if (rc != NMI_OK) return rc;
        *healed = (int32_t)n[nmi::kPixHealed];
    }
    return NMI_OK;
}

int nmi_pix_heal_counts(nmi_ctx *ctx, int32_t *timeouts, int32_t *count_test)
{
    if (!ctx) return NMI_ERR_INVALID_ARGUMENT;
    uint32_t n[nmi::kPixHealWords];
    const int rc = read_pix_heal(ctx, n);
    if (rc != NMI_OK) return rc;
    if (timeouts) *timeouts = (int32_t)n[nmi::kPixHealTimeouts];
    if (count_test) *count_test = (int32_t)n[nmi::kPixHealCountTest];
    return NMI_OK;
}

int nmi_search_grid(nmi_ctx *ctx, const uint8_t *render_stack, int32_t S, const uint8_t *warp_stack, int32_t Wn,
                    float *d_ratings, int64_t *h_best_index, float *h_best_score)
{
    uint64_t key = 0;
    int rc = nmi_search_grid_shard(ctx, render_stack, S, 0, S, warp_stack, Wn, d_ratings, nullptr, &key);
    if (rc != NMI_OK) return rc;
    return nmi_key_unpack(key, h_best_index, h_best_score);
}

int nmi_eval_pair_debug(nmi_ctx *ctx, const uint8_t *render, const uint8_t *warped, float *h_score, uint32_t *d_joint,
                        uint32_t *d_hist_render, uint32_t *d_hist_warped, float *d_sums)
{
    if (!ctx || !render || !warped || !h_score) return NMI_ERR_INVALID_ARGUMENT;
    ctx->detail.clear();
    DeviceGuard guard(ctx->device);
    const bool dbg = d_joint || d_hist_render || d_hist_warped || d_sums;
    SearchRequest rq = SearchRequest::block(render, 1, 0, 1, warped, 1);
    rq.d_ratings = ctx->d_pair_rating.as<float>();
    rq.post_score = true;
    rq.dbg_joint = d_joint;
    rq.dbg_h1 = d_hist_render;
    rq.dbg_h2 = d_hist_warped;
    rq.dbg_sums = d_sums;
    int rc = enqueue_grid(ctx, rq);
    if (rc != NMI_OK) return rc;
    if (ctx->result_path == 1) {
        // kernel.cu:100 copies the score back with a blocking cudaMemcpy; here the scoring lane stores
        // (score bits | call number << 32) into pinned host memory and the call polls that word (~10 us less per call).
        unsigned long long word = 0;
        rc = wait_word(ctx, ctx->score_mailbox.as<unsigned long long>(), 0xFFFFFFFF00000000ull, (unsigned long long)ctx->pair_seq << 32, &word);
        if (rc == NMI_OK && split_timed_out(ctx)) {
            rc = nmi_eval_pair_debug(ctx, render, warped, h_score, d_joint, d_hist_render, d_hist_warped, d_sums);
            if (rc == NMI_OK) ctx->detail = kSplitTimeoutNote;
            return rc;
        }
        if (rc == NMI_OK) {
            const uint32_t bits = (uint32_t)word;
            memcpy(h_score, &bits, sizeof bits);
            if (dbg) NMI_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // the exported histograms must be complete
            return NMI_OK;
        }
        if (rc != NMI_ERR_NOT_READY) return rc;
    }
    NMI_HIP_TRY(ctx, hipMemcpyAsync(h_score, ctx->d_pair_rating.as<>(), sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    NMI_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (split_timed_out(ctx)) {
        rc = nmi_eval_pair_debug(ctx, render, warped, h_score, d_joint, d_hist_render, d_hist_warped, d_sums);
        if (rc == NMI_OK) ctx->detail = kSplitTimeoutNote;
        return rc;
    }
    return NMI_OK;
}

int nmi_eval_pairs(nmi_ctx *ctx, const uint8_t *const *h_renders, const uint8_t *const *h_warps, int32_t n, float *h_scores)
{
    if (!ctx || n < 0 || (n > 0 && (!h_renders || !h_warps || !h_scores))) return NMI_ERR_INVALID_ARGUMENT;
    for (int i = 0; i < n; ++i)
        if (!h_renders[i] || !h_warps[i]) return NMI_ERR_INVALID_ARGUMENT;
    ctx->detail.clear();
    if (n == 0) return NMI_OK;
    DeviceGuard guard(ctx->device);
    // launches of at most compute_units / 4 pairs (4 row parts each); small batches get more parts per pair
    const int min_parts = ctx->split_mode > 1 ? ctx->split_mode : 4;
    const int cus = ctx->workgroups > 0 && ctx->workgroups < ctx->compute_units ? ctx->workgroups : ctx->compute_units;
    const int per_launch = cus / min_parts > 0 ? ((cus / min_parts) & ~7) > 0 ? (cus / min_parts) & ~7 : 1 : 1;
    // Decided BEFORE anything is launched: does a split form exist for every chunk of this batch (none does with
    // NMI_OPT_WORKGROUPS below 16, with NMI_OPT_SPLIT 0, or while the split forms are paused after a timeout)?
    if ((int64_t)n > (int64_t)per_launch * 128) {  // the timeout ring answers for at most kSplitRing launches in flight
        for (int off = 0; off < n; off += per_launch * 128) {
            const int m = n - off < per_launch * 128 ? n - off : per_launch * 128;
            const int rc = nmi_eval_pairs(ctx, h_renders + off, h_warps + off, m, h_scores + off);
            if (rc != NMI_OK) return rc;
        }
        return NMI_OK;
    }
    bool split_ok = true;
    for (int off = 0; split_ok && off < n; off += per_launch) {
        nmi::PlanInputs in = plan_inputs(ctx, nmi::SearchForm::plain, n - off < per_launch ? n - off : per_launch, nmi::GridArgs{});
        in.pair_pointers = in.split_checked = true;
        split_ok = !nmi::plan_search(in).unsupported;
    }
    if (!split_ok) {  // one pair at a time (nmi_eval_pair consumes the cooldown)
        for (int i = 0; i < n; ++i) {
            const int rc = nmi_eval_pair(ctx, h_renders[i], h_warps[i], &h_scores[i]);
            if (rc != NMI_OK) return rc;
        }
        return NMI_OK;
    }
    // pointer tables (pinned, device-mapped) and the scores (device), grown on demand
    NMI_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // growing or not: an earlier batch may still be reading the tables
    if (n > ctx->pairs_cap) {
        ctx->pairs_cap = 0;
        const int cap = n > 256 ? n : 256;
        NMI_HIP_TRY(ctx, ctx->pair_table.grow((size_t)cap * 2 * sizeof(void *), nmi_mem::kPosted));
        NMI_HIP_TRY(ctx, ctx->d_pair_scores.grow((size_t)cap * sizeof(float)));
        ctx->pairs_cap = cap;
    }
    const uint8_t **h_pair_table = ctx->pair_table.as<const uint8_t *>(), **d_pair_table = ctx->pair_table.device<const uint8_t *>();
    float *d_pair_scores = ctx->d_pair_scores.as<float>();
    for (int i = 0; i < n; ++i) {
        h_pair_table[i] = h_renders[i];
        h_pair_table[ctx->pairs_cap + i] = h_warps[i];
    }
    SearchLaunch launches[128];  // (the batch was cut to at most that many above)
    int n_launches = 0;
    for (int off = 0; off < n; off += per_launch) {
        const int m = n - off < per_launch ? n - off : per_launch;
        SearchRequest rq = SearchRequest::block(h_renders[off], m, 0, m, h_warps[off], 1);
        rq.d_ratings = d_pair_scores + off;
        rq.pair_renders = d_pair_table + off;
        rq.pair_warps = d_pair_table + ctx->pairs_cap + off;
        rq.pair_renders_host = h_renders + off;
        rq.pair_warps_host = h_warps + off;
        const int rc = enqueue_grid(ctx, rq, &launches[n_launches]);
        if (rc != NMI_OK) return rc;  // (NMI_ERR_UNSUPPORTED, before any launch, had no split form fitted after all)
        ++n_launches;
    }
    NMI_HIP_TRY(ctx, hipMemcpyAsync(h_scores, d_pair_scores, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    NMI_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    bool failed = false;  // every launch of the batch answers for itself
    for (int i = 0; i < n_launches; ++i) failed = split_launch_failed(ctx, launches[i]) || failed;
    if (failed) {  // now one pair at a time, through nmi_grid_kernel
        const int rc = nmi_eval_pairs(ctx, h_renders, h_warps, n, h_scores);
        if (rc == NMI_OK) ctx->detail = kSplitTimeoutNote;
        return rc;
    }
    return NMI_OK;
}

int nmi_eval_pair(nmi_ctx *ctx, const uint8_t *render, const uint8_t *warped, float *h_score)
{
    return nmi_eval_pair_debug(ctx, render, warped, h_score, nullptr, nullptr, nullptr, nullptr);
}

}  // extern "C"
