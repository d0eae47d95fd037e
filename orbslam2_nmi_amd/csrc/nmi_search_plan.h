// nmi_search_plan.h -- which kernel scores a search, decided in one pure function.  Nothing here touches the device or a
// context: plan_search maps the scalars of a call (PlanInputs) to a SearchPlan, and the callers (enqueue_grid,
// enqueue_grid_mask, level_capture, nmi_eval_pairs' pre-check) act on it.  The grid-size helpers the kernels share with the
// host live here too (nmi_split_kernel.hip, nmi_pix_device.h include this file).  tests/native/search_plan.cpp holds the
// policy for 256 compute units as a literal table.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define NMI_PLAN_HD __host__ __device__
#else
#define NMI_PLAN_HD
#endif

namespace nmi {

// Grid of a split launch (one unit per workgroup): candidates rounded up to 8 (the units are dealt XCD by XCD), except below 8
// candidates of 8 row parts, where row part j sits on XCD j as it is.
NMI_PLAN_HD inline bool split_exact_grid(int total, int parts) { return total < 8 && parts == 8; }  // (row part j on XCD j needs 8 of them)
NMI_PLAN_HD inline int split_workgroups(int candidates, int parts, int pix_parts)
{
    return (split_exact_grid(candidates, parts) ? candidates : ((candidates + 7) / 8) * 8) * parts * pix_parts;
}
constexpr int kPixMaxRanges = 5;  // nmi_pix_kernel: a wave's 64 lanes poll 16 granules of each of at most 4 helpers

enum class SearchForm { plain, masked, level };  // masked: the masked and covered searches; level: a captured level's search node
enum class SearchKernel { none, grid, split, pix, few_levels };  // none: nothing to score; few_levels: followed by the gated grid kernel

struct PlanInputs {
    int compute_units = 0;
    int workgroups = 0;        // NMI_OPT_WORKGROUPS (0: one per compute unit)
    int hist_variant = 3;
    int split_mode = -1;       // NMI_OPT_SPLIT
    int split_pixels = -1;     // NMI_OPT_SPLIT_PIXELS
    int shift = 0;
    bool use_bg = true;
    int phase_mask = 3;
    int content_path = -1;     // NMI_OPT_CONTENT_PATH
    bool xcd_tiling = true;
    bool cooldown = false;     // split forms paused after a timeout (split_cooldown > 0)
    bool few_hint = false;     // the most recent content probe found few distinct intensities
    int64_t total = 0;         // candidates of this launch
    int width = 0, npix = 0;
    bool vec_ok = false;       // rows are whole aligned 16-byte chunks
    bool debug_exports = false, stamps = false, pair_pointers = false;
    bool split_checked = false;  // somebody looks for a split-kernel timeout after this launch
    SearchForm form = SearchForm::plain;
};

struct SearchPlan {
    SearchKernel kind = SearchKernel::none;
    int parts = 0;             // row parts per candidate (split), else 0
    int pix_parts = 1;         // ... and pixel ranges of the split kernel
    int pix = 0;               // pixel ranges per candidate of the pixel-range kernels, else 0
    int workgroups = 0;        // grid of the launch (masked and level forms: of their grid kernel; their pixel-range launchers size themselves)
    int phase_mask = 3;        // what the kernel gets: the masked and level forms pass on the hand-off test hook (bit 9) only
    bool order_table = false;  // the launch reads an XCD-aware visiting order
    bool shared_order = false; // ... the one that keeps a warp per workgroup (build_search_order): nmi_grid_kernel's own launches only
    bool probe = false;        // the launch doubles as a content probe (GridArgs::plan)
    bool scratch = false;      // the launch is the pipelined kernel's (ablation build): it needs the drained-counter slabs
    bool used_cooldown = false;  // a split form was held back by the pause: the caller takes one unit off it
    bool read_hint = false;    // the few-levels hint was consulted: the caller keeps the refreshed value
    bool unsupported = false;  // per-pair pointers, and no split form for them (NMI_ERR_UNSUPPORTED)
};

// The workgroups a launch may use, and the grid of a one-workgroup-per-candidate launch of `total` candidates.
inline int plan_cap(int workgroups_option, int compute_units) { return workgroups_option > 0 ? workgroups_option : compute_units; }
inline int grid_workgroups(int64_t total, int workgroups_option, int compute_units)
{
    const int cap = plan_cap(workgroups_option, compute_units);
    return (int)(total < cap ? total : cap);
}

// How the split kernel should cut each candidate of a launch of `total` candidates on `cap` workgroups: *parts row
// parts and *pix_parts pixel ranges.  *parts = 0: use the one-workgroup-per-candidate kernel.  Automatic choice (256
// CUs): up to 8 candidates 8 x 4, up to 16: 8 x 2, up to 32: 4 x 2, up to 64: 4 x 1 -- a part's time is its pixel stream
// (>= 12 us for a whole 640x480 pair whatever the number of row parts), so pixel ranges come first and 2 row parts,
// measured no faster than none, are available on request only.
inline void plan_split(const PlanInputs &in, int cap, int *parts, int *pix_parts)
{
    *parts = 0;
    *pix_parts = 1;
    const int64_t total = in.total;
    if (cap > in.compute_units) cap = in.compute_units;  // all workgroups of a split launch must be resident at once
    if (in.hist_variant != 3 || in.split_mode == 0 || in.split_mode == 1 || total <= 0 || total > cap) return;
    auto fits = [&](int k, int p) { return split_workgroups((int)total, k, p) <= cap; };
    auto exists = [](int k, int p) { return p == 1 || (k == 8 && (p == 2 || p == 4)) || (k == 4 && p == 2); };
    const int want_p = in.split_pixels;  // -1 automatic, 1 never, 2 / 4 that many when it fits
    if (in.split_mode > 0) {
        const int k = in.split_mode;
        if (!fits(k, 1)) return;
        *parts = k;
        if (want_p == 1) return;
        for (int p = 4; p >= 2; p >>= 1)
            if ((want_p == -1 || want_p == p) && exists(k, p) && fits(k, p)) {
                *pix_parts = p;
                return;
            }
        return;
    }
    static const int order[][2] = {{8, 4}, {8, 2}, {4, 2}, {8, 1}, {4, 1}};
    for (const auto &kp : order) {
        if (kp[1] > 1 && want_p != -1 && want_p != kp[1]) continue;
        if (fits(kp[0], kp[1])) {
            *parts = kp[0];
            *pix_parts = kp[1];
            return;
        }
    }
}

// Pixel ranges per candidate for the pixel-range kernels (nmi_pix_kernel.hip and its masked and covered forms), 0 = another
// kernel.  The owner of a candidate adds its P - 1 helpers' histograms to its own and waits for the slowest of them, so P grows
// only while the histogram phase (21 us / P at 640x480) shrinks faster: automatic choice 3 up to 85 candidates, 2 up to 128 (256
// CUs; measured, with 4 and 5: profiles/r04_a/small_grid_time.txt); smaller grids keep the row-split forms, larger ones have no
// CU to spare.  NMI_OPT_SPLIT 1 + NMI_OPT_SPLIT_PIXELS P forces P wherever it fits.
inline int plan_pix(const PlanInputs &in, int cap)
{
    const int64_t total = in.total;
    const bool stamps = in.stamps && in.form == SearchForm::plain;  // (the other forms have no stamped kernel)
    if (cap > in.compute_units) cap = in.compute_units;  // (an owner that waits for a CU starts a second round)
    if (in.hist_variant != 3 || in.width < 32 || (in.shift != 0 && !in.use_bg) || in.pair_pointers || total <= 0) return 0;
    if ((in.phase_mask & ~512) != 3 || (stamps && in.split_mode != 1)) return 0;
    if (in.split_mode == 1) {
        const int p = in.split_pixels;
        return (p >= 2 && p <= kPixMaxRanges && total * p <= cap) ? p : 0;
    }
    if (in.split_mode != -1 || in.split_pixels != -1 || total * 2 > cap) return 0;
    const int p = (int)(cap / total);
    // Frames whose rows are not whole aligned 16-byte chunks (width % 16 != 0, unaligned stacks): the row-split kernel would
    // read them byte by byte, this one has the unaligned-row form -- so small grids and single pairs come here too, with more ranges
    if (!in.vec_ok) return p > kPixMaxRanges ? kPixMaxRanges : p;
    if (total <= 32) return 0;
    return p > 3 ? 3 : p;
}

inline SearchPlan plan_search(const PlanInputs &in)
{
    SearchPlan plan;
    if (in.total <= 0) return plan;
    const int cap = plan_cap(in.workgroups, in.compute_units);
    plan.workgroups = grid_workgroups(in.total, in.workgroups, in.compute_units);
    plan.pix = plan_pix(in, cap);  // mid-size grids: pixel ranges (no residence condition, heals itself)
    if (in.form != SearchForm::plain) {
        // masked, covered and level searches: their grid kernel or its pixel-range form, by the plain search's rules and controls
        plan.kind = plan.pix ? SearchKernel::pix : SearchKernel::grid;
        plan.phase_mask = plan.pix ? 3 | (in.phase_mask & 512) : 3;
        plan.order_table = !plan.pix && (in.form == SearchForm::level || (in.xcd_tiling && in.total <= (1ll << 24)));
        return plan;
    }
    plan.phase_mask = in.phase_mask;
    // the split kernel's consumers wait for their producers inside the launch: all its workgroups must be able to run at
    // once, i.e. no more of them than compute units (each takes a whole CU)
    plan_split(in, cap, &plan.parts, &plan.pix_parts);
    if (plan.pix_parts > 1 && in.npix >= (1 << 24)) plan.pix_parts = 1;  // block granules hold 24-bit counts
    if (plan.pix) plan.parts = 0;
    if (plan.parts && !in.split_checked) plan.parts = 0;  // enqueue-only call: nobody would notice a timed-out hand-off, so no split kernel
    if (plan.parts && in.cooldown) {  // after a timeout: nmi_grid_kernel for a while, then the split forms again
        plan.used_cooldown = true;
        plan.parts = 0;
    }
    if (!plan.parts) plan.pix_parts = 1;
    // Few-levels path (nmi_fewlevels_kernel.hip).  The decision rests on what the most recent probe of a search's stacks
    // found (frames and renders of consecutive searches look alike); it is only a matter of speed, because the probe that
    // goes with every few-levels launch hands the search back to nmi_grid_kernel (its gated launch) when this search's
    // stacks do not qualify.
    plan.read_hint = !plan.parts && !(plan.pix && in.split_mode == 1) && in.vec_ok && (in.shift == 0 || in.use_bg) && in.hist_variant == 3 &&
                     in.phase_mask == 3 && !in.debug_exports && !in.pair_pointers && !in.stamps && in.content_path != 0;
    const bool few = plan.read_hint && (in.content_path == 1 || in.few_hint);
    if (few) plan.pix = 0;  // few distinct intensities: the few-levels kernels are the faster ones at any grid size
    if (in.pair_pointers && !plan.parts) {  // per-pair pointers exist in the split kernel only
        plan.unsupported = true;
        plan.workgroups = 0;
        return plan;
    }
    if (plan.parts) {
        plan.kind = SearchKernel::split;
        plan.workgroups = split_workgroups((int)in.total, plan.parts, plan.pix_parts);
    } else if (plan.pix) {
        plan.kind = SearchKernel::pix;
        plan.workgroups = (int)in.total * plan.pix;
    } else {
        plan.kind = few ? SearchKernel::few_levels : SearchKernel::grid;
        plan.order_table = in.xcd_tiling && in.total <= (1ll << 24);  // 4 B per candidate
        plan.shared_order = plan.order_table && !few;
    }
    plan.scratch = in.hist_variant == 4;
    plan.probe = !plan.parts && in.hist_variant == 3 && in.content_path != 0;  // (the few-levels launch carries its own probe's plan)
    return plan;
}

// ---- visiting orders (host) ----------------------------------------------------------------------------------------------------
// Workgroup b of a launch of `grid` workgroups visits the ordinals slot, slot + grid, slot + 2 grid, ... of the order table, where
// slot = slot_in_round(b, grid) (nmi_grid_device.h); workgroups are dealt to the 8 XCDs round-robin.

// Today's tiles: kTileW warps x kTileS renders (32 candidates = the 32 workgroups one XCD runs at a time), tile after tile; within
// a tile render-fastest.  Independent of the grid.
inline void build_tile_order(int S, int Wn, int *order)
{
    const int tile_s = S >= 8 ? 8 : (S >= 4 ? 4 : (S >= 2 ? 2 : 1)), tile_w = 32 / tile_s;
    int64_t o = 0;
    for (int w0 = 0; w0 < Wn; w0 += tile_w)
        for (int s0 = 0; s0 < S; s0 += tile_s)
            for (int w = w0; w < w0 + tile_w && w < Wn; ++w)
                for (int s = s0; s < s0 + tile_s && s < S; ++s) order[o++] = w * S + s;
}

// The slot at position `pos` when the slots of a launch are listed XCD by XCD.  A grid that is a multiple of 8: slot_in_round has
// done that already (slots [x grid/8, (x + 1) grid/8) run on XCD x).  Any other grid: slot = workgroup, XCD = slot % 8.
inline int order_slot_at(int pos, int grid)
{
    if ((grid & 7) == 0) return pos;
    for (int x = 0; x < 8; ++x) {
        const int n = (grid - x + 7) / 8;
        if (pos < n) return x + 8 * pos;
        pos -= n;
    }
    return -1;
}

// A visiting order in which every workgroup of a launch of `grid` workgroups keeps ONE warp: the candidates at the ordinals
// slot + k grid share w, so that nmi_grid_kernel forms the frame marginal once per workgroup.  With R = ceil(S Wn / grid) rounds, a
// slot has R candidates (the first A slots) or R - 1 (the other B); warp w gets x_w slots of the first kind and y_w of the second
// with R x_w + (R - 1) y_w = S, i.e. y_w = y0 + j_w R with y0 = -S mod R, and the j_w add up so that the y_w use up B (spread over
// the last warps, one R at a time).  Slots are handed out in XCD order (order_slot_at), warp after warp, and slot t of a warp's m = x + y slots
// takes render k m + t in round k: the 32 workgroups of an XCD then hold 32 / m + 1 or + 2 warps and, in one round, the same m
// renders -- 13 or 14 images for 27 x 27 on 243 or 256 workgroups (m = 9, 10), where the tiles hold 12.
// -> false, `order` untouched, where no such split exists (one round only, S or Wn of 1, S not reachable from R and R - 1).
inline bool build_shared_order(int S, int Wn, int grid, int *order)
{
    const int64_t total = (int64_t)S * Wn;
    if (S < 2 || Wn < 2 || grid < 1 || total <= grid) return false;
    const int R = (int)((total + grid - 1) / grid);               // rounds; >= 2
    const int A = (int)(total - (int64_t)(R - 1) * grid);         // slots [0, A) have R candidates, [A, grid) R - 1
    const int B = grid - A;
    const int y0 = (R - S % R) % R;
    if ((int64_t)y0 * (R - 1) > S) return false;
    const int x0 = (S - y0 * (R - 1)) / R;                        // (exact)
    const int64_t rest = (int64_t)B - (int64_t)Wn * y0;
    if (rest < 0 || rest % R) return false;
    const int64_t J = rest / R;
    const int jmax = x0 / (R - 1);
    if (J > (int64_t)Wn * jmax) return false;
    const int j_all = (int)(J / Wn), j_more = (int)(J % Wn);     // the last j_more warps take one more
    // The slots with R candidates go to the warps in rising order and those with R - 1 in falling order, so that the one XCD that
    // holds slots of both kinds holds them of the same (last) warps.
    for (int kind = 0; kind < 2; ++kind) {
        int pos = 0;
        for (int v = 0; v < Wn; ++v) {
            const int w = kind == 0 ? v : Wn - 1 - v;
            const int j = j_all + (w >= Wn - j_more ? 1 : 0);
            const int x = x0 - j * (R - 1), y = y0 + j * R, m = x + y;
            for (int t = kind == 0 ? 0 : x; t < (kind == 0 ? x : m); ++t) {
                int slot;
                do slot = order_slot_at(pos++, grid);
                while ((slot < A) != (kind == 0));
                const int n = kind == 0 ? R : R - 1;
                for (int k = 0; k < n; ++k) order[slot + (int64_t)k * grid] = w * S + k * m + t;
            }
        }
    }
    return true;
}

// The order a plain nmi_grid_kernel search of an S x Wn grid on `grid` workgroups reads: one warp per workgroup where that exists,
// today's tiles otherwise.
inline void build_search_order(int S, int Wn, int grid, int *order)
{
    if (!build_shared_order(S, Wn, grid, order)) build_tile_order(S, Wn, order);
}

}  // namespace nmi
