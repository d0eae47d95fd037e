// CPU test of the search dispatch policy (csrc/nmi_search_plan.h): plan_search against a literal table of boundary cases for
// 256 compute units.  The table is the documented policy: its values were recorded from the functions plan_search replaced
// (choose_split, choose_pix and enqueue_grid's override chain), not read off plan_search.  Stand-alone: g++ -fsanitize=address,undefined.
#include <stdio.h>

#include "nmi_search_plan.h"

using F = nmi::SearchForm;
using K = nmi::SearchKernel;

struct Case {
    const char *name;
    F form;
    long long total;
    int width, vec_ok, split_mode, split_pixels, cooldown, checked, pairs, hint, content_path;
    // expected
    K kind;
    int parts, pix_parts, pix, workgroups, order_table, probe, used_cooldown, unsupported;
};

// 640 x 480 frames unless the width says otherwise; NMI_OPT_WORKGROUPS 0, 256 bins, background rule on, phase mask 3.
static const Case kCases[] = {
    {"aligned, blocking, 1", F::plain, 1, 640, 1, -1, -1, 0, 1, 0, 0, -1, /* -> */ K::split, 8, 4, 0, 32, 0, 0, 0, 0},
    {"aligned, blocking, 8", F::plain, 8, 640, 1, -1, -1, 0, 1, 0, 0, -1, /* -> */ K::split, 8, 4, 0, 256, 0, 0, 0, 0},
    {"aligned, blocking, 9", F::plain, 9, 640, 1, -1, -1, 0, 1, 0, 0, -1, /* -> */ K::split, 8, 2, 0, 256, 0, 0, 0, 0},
    {"aligned, blocking, 16", F::plain, 16, 640, 1, -1, -1, 0, 1, 0, 0, -1, /* -> */ K::split, 8, 2, 0, 256, 0, 0, 0, 0},
    {"aligned, blocking, 17", F::plain, 17, 640, 1, -1, -1, 0, 1, 0, 0, -1, /* -> */ K::split, 4, 2, 0, 192, 0, 0, 0, 0},
    {"aligned, blocking, 32", F::plain, 32, 640, 1, -1, -1, 0, 1, 0, 0, -1, /* -> */ K::split, 4, 2, 0, 256, 0, 0, 0, 0},
    {"aligned, blocking, 33", F::plain, 33, 640, 1, -1, -1, 0, 1, 0, 0, -1, /* -> */ K::pix, 0, 1, 3, 99, 0, 1, 0, 0},
    {"aligned, blocking, 64", F::plain, 64, 640, 1, -1, -1, 0, 1, 0, 0, -1, /* -> */ K::pix, 0, 1, 3, 192, 0, 1, 0, 0},
    {"aligned, blocking, 65", F::plain, 65, 640, 1, -1, -1, 0, 1, 0, 0, -1, /* -> */ K::pix, 0, 1, 3, 195, 0, 1, 0, 0},
    {"aligned, blocking, 85", F::plain, 85, 640, 1, -1, -1, 0, 1, 0, 0, -1, /* -> */ K::pix, 0, 1, 3, 255, 0, 1, 0, 0},
    {"aligned, blocking, 86", F::plain, 86, 640, 1, -1, -1, 0, 1, 0, 0, -1, /* -> */ K::pix, 0, 1, 2, 172, 0, 1, 0, 0},
    {"aligned, blocking, 128", F::plain, 128, 640, 1, -1, -1, 0, 1, 0, 0, -1, /* -> */ K::pix, 0, 1, 2, 256, 0, 1, 0, 0},
    {"aligned, blocking, 129", F::plain, 129, 640, 1, -1, -1, 0, 1, 0, 0, -1, /* -> */ K::grid, 0, 1, 0, 129, 1, 1, 0, 0},
    {"aligned, blocking, 256", F::plain, 256, 640, 1, -1, -1, 0, 1, 0, 0, -1, /* -> */ K::grid, 0, 1, 0, 256, 1, 1, 0, 0},
    {"aligned, blocking, 257", F::plain, 257, 640, 1, -1, -1, 0, 1, 0, 0, -1, /* -> */ K::grid, 0, 1, 0, 256, 1, 1, 0, 0},
    {"unaligned rows, blocking, 1", F::plain, 1, 641, 0, -1, -1, 0, 1, 0, 0, -1, /* -> */ K::pix, 0, 1, 5, 5, 0, 1, 0, 0},
    {"unaligned rows, blocking, 8", F::plain, 8, 641, 0, -1, -1, 0, 1, 0, 0, -1, /* -> */ K::pix, 0, 1, 5, 40, 0, 1, 0, 0},
    {"unaligned rows, blocking, 9", F::plain, 9, 641, 0, -1, -1, 0, 1, 0, 0, -1, /* -> */ K::pix, 0, 1, 5, 45, 0, 1, 0, 0},
    {"unaligned rows, blocking, 16", F::plain, 16, 641, 0, -1, -1, 0, 1, 0, 0, -1, /* -> */ K::pix, 0, 1, 5, 80, 0, 1, 0, 0},
    {"unaligned rows, blocking, 17", F::plain, 17, 641, 0, -1, -1, 0, 1, 0, 0, -1, /* -> */ K::pix, 0, 1, 5, 85, 0, 1, 0, 0},
    {"unaligned rows, blocking, 32", F::plain, 32, 641, 0, -1, -1, 0, 1, 0, 0, -1, /* -> */ K::pix, 0, 1, 5, 160, 0, 1, 0, 0},
    {"unaligned rows, blocking, 33", F::plain, 33, 641, 0, -1, -1, 0, 1, 0, 0, -1, /* -> */ K::pix, 0, 1, 5, 165, 0, 1, 0, 0},
    {"unaligned rows, blocking, 64", F::plain, 64, 641, 0, -1, -1, 0, 1, 0, 0, -1, /* -> */ K::pix, 0, 1, 4, 256, 0, 1, 0, 0},
    {"unaligned rows, blocking, 65", F::plain, 65, 641, 0, -1, -1, 0, 1, 0, 0, -1, /* -> */ K::pix, 0, 1, 3, 195, 0, 1, 0, 0},
    {"unaligned rows, blocking, 85", F::plain, 85, 641, 0, -1, -1, 0, 1, 0, 0, -1, /* -> */ K::pix, 0, 1, 3, 255, 0, 1, 0, 0},
    {"unaligned rows, blocking, 86", F::plain, 86, 641, 0, -1, -1, 0, 1, 0, 0, -1, /* -> */ K::pix, 0, 1, 2, 172, 0, 1, 0, 0},
    {"unaligned rows, blocking, 128", F::plain, 128, 641, 0, -1, -1, 0, 1, 0, 0, -1, /* -> */ K::pix, 0, 1, 2, 256, 0, 1, 0, 0},
    {"unaligned rows, blocking, 129", F::plain, 129, 641, 0, -1, -1, 0, 1, 0, 0, -1, /* -> */ K::grid, 0, 1, 0, 129, 1, 1, 0, 0},
    {"unaligned rows, blocking, 256", F::plain, 256, 641, 0, -1, -1, 0, 1, 0, 0, -1, /* -> */ K::grid, 0, 1, 0, 256, 1, 1, 0, 0},
    {"unaligned rows, blocking, 257", F::plain, 257, 641, 0, -1, -1, 0, 1, 0, 0, -1, /* -> */ K::grid, 0, 1, 0, 256, 1, 1, 0, 0},
    {"width 16, 1", F::plain, 1, 16, 0, -1, -1, 0, 1, 0, 0, -1, /* -> */ K::split, 8, 4, 0, 32, 0, 0, 0, 0},
    {"width 16, 40", F::plain, 40, 16, 0, -1, -1, 0, 1, 0, 0, -1, /* -> */ K::split, 4, 1, 0, 160, 0, 0, 0, 0},
    {"width 16, 300", F::plain, 300, 16, 0, -1, -1, 0, 1, 0, 0, -1, /* -> */ K::grid, 0, 1, 0, 256, 1, 1, 0, 0},
    {"NMI_OPT_SPLIT 0, 1", F::plain, 1, 640, 1, 0, -1, 0, 1, 0, 0, -1, /* -> */ K::grid, 0, 1, 0, 1, 1, 1, 0, 0},
    {"NMI_OPT_SPLIT 0, 40", F::plain, 40, 640, 1, 0, -1, 0, 1, 0, 0, -1, /* -> */ K::grid, 0, 1, 0, 40, 1, 1, 0, 0},
    {"NMI_OPT_SPLIT 0, 300", F::plain, 300, 640, 1, 0, -1, 0, 1, 0, 0, -1, /* -> */ K::grid, 0, 1, 0, 256, 1, 1, 0, 0},
    {"NMI_OPT_SPLIT 1, 2 ranges, 1", F::plain, 1, 640, 1, 1, 2, 0, 1, 0, 0, -1, /* -> */ K::pix, 0, 1, 2, 2, 0, 1, 0, 0},
    {"NMI_OPT_SPLIT 1, 2 ranges, 40", F::plain, 40, 640, 1, 1, 2, 0, 1, 0, 0, -1, /* -> */ K::pix, 0, 1, 2, 80, 0, 1, 0, 0},
    {"NMI_OPT_SPLIT 1, 2 ranges, 128", F::plain, 128, 640, 1, 1, 2, 0, 1, 0, 0, -1, /* -> */ K::pix, 0, 1, 2, 256, 0, 1, 0, 0},
    {"NMI_OPT_SPLIT 1, 2 ranges, 129", F::plain, 129, 640, 1, 1, 2, 0, 1, 0, 0, -1, /* -> */ K::grid, 0, 1, 0, 129, 1, 1, 0, 0},
    {"NMI_OPT_SPLIT 1, 8 ranges (more than the kernel has), 1", F::plain, 1, 640, 1, 1, 8, 0, 1, 0, 0, -1, /* -> */ K::grid, 0, 1, 0, 1, 1, 1, 0, 0},
    {"NMI_OPT_SPLIT 1, 8 ranges (more than the kernel has), 40", F::plain, 40, 640, 1, 1, 8, 0, 1, 0, 0, -1, /* -> */ K::grid, 0, 1, 0, 40, 1, 1, 0, 0},
    {"NMI_OPT_SPLIT 8, 1", F::plain, 1, 640, 1, 8, -1, 0, 1, 0, 0, -1, /* -> */ K::split, 8, 4, 0, 32, 0, 0, 0, 0},
    {"NMI_OPT_SPLIT 8, 8", F::plain, 8, 640, 1, 8, -1, 0, 1, 0, 0, -1, /* -> */ K::split, 8, 4, 0, 256, 0, 0, 0, 0},
    {"NMI_OPT_SPLIT 8, 9", F::plain, 9, 640, 1, 8, -1, 0, 1, 0, 0, -1, /* -> */ K::split, 8, 2, 0, 256, 0, 0, 0, 0},
    {"NMI_OPT_SPLIT 8, 16", F::plain, 16, 640, 1, 8, -1, 0, 1, 0, 0, -1, /* -> */ K::split, 8, 2, 0, 256, 0, 0, 0, 0},
    {"NMI_OPT_SPLIT 8, 17", F::plain, 17, 640, 1, 8, -1, 0, 1, 0, 0, -1, /* -> */ K::split, 8, 1, 0, 192, 0, 0, 0, 0},
    {"NMI_OPT_SPLIT 8, 32", F::plain, 32, 640, 1, 8, -1, 0, 1, 0, 0, -1, /* -> */ K::split, 8, 1, 0, 256, 0, 0, 0, 0},
    {"NMI_OPT_SPLIT 8, 33", F::plain, 33, 640, 1, 8, -1, 0, 1, 0, 0, -1, /* -> */ K::grid, 0, 1, 0, 33, 1, 1, 0, 0},
    {"split forms paused, 1", F::plain, 1, 640, 1, -1, -1, 1, 1, 0, 0, -1, /* -> */ K::grid, 0, 1, 0, 1, 1, 1, 1, 0},
    {"split forms paused, 9", F::plain, 9, 640, 1, -1, -1, 1, 1, 0, 0, -1, /* -> */ K::grid, 0, 1, 0, 9, 1, 1, 1, 0},
    {"split forms paused, 40", F::plain, 40, 640, 1, -1, -1, 1, 1, 0, 0, -1, /* -> */ K::pix, 0, 1, 3, 120, 0, 1, 0, 0},
    {"split forms paused, 300", F::plain, 300, 640, 1, -1, -1, 1, 1, 0, 0, -1, /* -> */ K::grid, 0, 1, 0, 256, 1, 1, 0, 0},
    {"enqueue-only, unchecked, 1", F::plain, 1, 640, 1, -1, -1, 0, 0, 0, 0, -1, /* -> */ K::grid, 0, 1, 0, 1, 1, 1, 0, 0},
    {"enqueue-only, unchecked, 9", F::plain, 9, 640, 1, -1, -1, 0, 0, 0, 0, -1, /* -> */ K::grid, 0, 1, 0, 9, 1, 1, 0, 0},
    {"enqueue-only, unchecked, 40", F::plain, 40, 640, 1, -1, -1, 0, 0, 0, 0, -1, /* -> */ K::pix, 0, 1, 3, 120, 0, 1, 0, 0},
    {"enqueue-only, unchecked, 300", F::plain, 300, 640, 1, -1, -1, 0, 0, 0, 0, -1, /* -> */ K::grid, 0, 1, 0, 256, 1, 1, 0, 0},
    {"per-pair pointers, 5", F::plain, 5, 640, 1, -1, -1, 0, 0, 1, 0, -1, /* -> */ K::split, 8, 4, 0, 160, 0, 0, 0, 0},
    {"per-pair pointers, 64", F::plain, 64, 640, 1, -1, -1, 0, 0, 1, 0, -1, /* -> */ K::split, 4, 1, 0, 256, 0, 0, 0, 0},
    {"per-pair pointers, NMI_OPT_SPLIT 0: NMI_ERR_UNSUPPORTED", F::plain, 5, 640, 1, 0, -1, 0, 1, 1, 0, -1, /* -> */ K::none, 0, 1, 0, 0, 0, 0, 0, 1},
    {"per-pair pointers, split forms paused: NMI_ERR_UNSUPPORTED", F::plain, 5, 640, 1, -1, -1, 1, 1, 1, 0, -1, /* -> */ K::none, 0, 1, 0, 0, 0, 0, 1, 1},
    {"per-pair pointers, 65 (no split form): NMI_ERR_UNSUPPORTED", F::plain, 65, 640, 1, -1, -1, 0, 1, 1, 0, -1, /* -> */ K::none, 0, 1, 0, 0, 0, 0, 0, 1},
    {"few-levels hint, 9", F::plain, 9, 640, 1, -1, -1, 0, 1, 0, 1, -1, /* -> */ K::split, 8, 2, 0, 256, 0, 0, 0, 0},
    {"few-levels hint, 40", F::plain, 40, 640, 1, -1, -1, 0, 1, 0, 1, -1, /* -> */ K::few_levels, 0, 1, 0, 40, 1, 1, 0, 0},
    {"few-levels hint, 300", F::plain, 300, 640, 1, -1, -1, 0, 1, 0, 1, -1, /* -> */ K::few_levels, 0, 1, 0, 256, 1, 1, 0, 0},
    {"few-levels hint, forced 2 ranges, 40", F::plain, 40, 640, 1, 1, 2, 0, 1, 0, 1, -1, /* -> */ K::pix, 0, 1, 2, 80, 0, 1, 0, 0},
    {"few-levels hint, unaligned rows, 40", F::plain, 40, 641, 0, -1, -1, 0, 1, 0, 1, -1, /* -> */ K::pix, 0, 1, 5, 200, 0, 1, 0, 0},
    {"NMI_OPT_CONTENT_PATH 1, no hint, 300", F::plain, 300, 640, 1, -1, -1, 0, 1, 0, 0, 1, /* -> */ K::few_levels, 0, 1, 0, 256, 1, 1, 0, 0},
    {"NMI_OPT_CONTENT_PATH 0, hint, 300", F::plain, 300, 640, 1, -1, -1, 0, 1, 0, 1, 0, /* -> */ K::grid, 0, 1, 0, 256, 1, 0, 0, 0},
    {"masked form, 40", F::masked, 40, 640, 1, -1, -1, 0, 1, 0, 0, -1, /* -> */ K::pix, 0, 1, 3, 40, 0, 0, 0, 0},
    {"masked form, 300", F::masked, 300, 640, 1, -1, -1, 0, 1, 0, 0, -1, /* -> */ K::grid, 0, 1, 0, 256, 1, 0, 0, 0},
    {"masked form, 36-pixel rows, 40", F::masked, 40, 36, 0, -1, -1, 0, 1, 0, 0, -1, /* -> */ K::pix, 0, 1, 5, 40, 0, 0, 0, 0},
};

int main()
{
    int bad = 0;
    for (const Case &c : kCases) {
        nmi::PlanInputs in;
        in.compute_units = 256;
        in.split_mode = c.split_mode;
        in.split_pixels = c.split_pixels;
        in.cooldown = c.cooldown != 0;
        in.few_hint = c.hint != 0;
        in.content_path = c.content_path;
        in.total = c.total;
        in.width = c.width;
        in.npix = c.width * 480;
        in.vec_ok = c.vec_ok != 0;
        in.pair_pointers = c.pairs != 0;
        in.split_checked = c.checked != 0 || c.pairs != 0;
        in.form = c.form;
        const nmi::SearchPlan p = nmi::plan_search(in);
        const bool ok = p.kind == c.kind && p.parts == c.parts && p.pix_parts == c.pix_parts && p.pix == c.pix && p.workgroups == c.workgroups &&
                        p.order_table == (c.order_table != 0) && p.probe == (c.probe != 0) && p.used_cooldown == (c.used_cooldown != 0) &&
                        p.unsupported == (c.unsupported != 0);
        if (!ok) {
            ++bad;
            printf("FAIL %s: kind %d parts %d x %d pix %d workgroups %d order %d probe %d cooldown %d unsupported %d\n", c.name, (int)p.kind, p.parts,
                   p.pix_parts, p.pix, p.workgroups, (int)p.order_table, (int)p.probe, (int)p.used_cooldown, (int)p.unsupported);
        }
    }
    // nothing to score; the 24-bit guard on the split kernel's pixel parts; the grid-size helpers the kernels share
    if (nmi::plan_search(nmi::PlanInputs{}).kind != K::none) ++bad, printf("FAIL empty search\n");
    nmi::PlanInputs big;
    big.compute_units = 256;
    big.total = 1;
    big.width = 4096;
    big.npix = 1 << 24;
    big.vec_ok = big.split_checked = true;
    const nmi::SearchPlan pb = nmi::plan_search(big);
    if (pb.kind != K::split || pb.parts != 8 || pb.pix_parts != 1 || pb.workgroups != 8) ++bad, printf("FAIL 2^24 pixels\n");
    if (nmi::split_workgroups(7, 8, 4) != 224 || nmi::split_workgroups(7, 4, 2) != 64 || nmi::split_workgroups(9, 8, 2) != 256) ++bad, printf("FAIL split_workgroups\n");
    if (nmi::grid_workgroups(300, 0, 256) != 256 || nmi::grid_workgroups(300, 16, 256) != 16 || nmi::grid_workgroups(5, 0, 256) != 5) ++bad, printf("FAIL grid_workgroups\n");
    if (bad) return 1;
    printf("search plan ok: %d cases\n", (int)(sizeof kCases / sizeof kCases[0]));
    return 0;
}
