// CPU test of the visiting orders (csrc/nmi_search_plan.h): build_search_order is a permutation at every shape and grid, keeps one
// warp per workgroup where the issue of this order asks for it, and is today's tile order -- written out again below, not called
// -- wherever no such split exists.  Stand-alone: g++ -fsanitize=address,undefined.
#include <stdio.h>

#include <vector>

#include "nmi_search_plan.h"

static int failures = 0;
#define CHECK(cond, ...)                  \
    do {                                  \
        if (!(cond)) {                    \
            ++failures;                   \
            printf("FAIL: " __VA_ARGS__); \
            printf("\n");                 \
        }                                 \
    } while (0)

// the tile order as it was before orders depended on the grid
static void tiles(int S, int Wn, std::vector<int> &order)
{
    const int tile_s = S >= 8 ? 8 : (S >= 4 ? 4 : (S >= 2 ? 2 : 1)), tile_w = 32 / tile_s;
    size_t o = 0;
    for (int w0 = 0; w0 < Wn; w0 += tile_w)
        for (int s0 = 0; s0 < S; s0 += tile_s)
            for (int w = w0; w < w0 + tile_w && w < Wn; ++w)
                for (int s = s0; s < s0 + tile_s && s < S; ++s) order[o++] = w * S + s;
}

static std::vector<int> order_of(int S, int Wn, int grid)
{
    std::vector<int> order((size_t)S * Wn, -1);  // (exactly S * Wn: a write past the table is ASan's to find)
    nmi::build_search_order(S, Wn, grid, order.data());
    return order;
}

static bool is_permutation(const std::vector<int> &order)
{
    std::vector<char> seen(order.size(), 0);
    for (int p : order) {
        if (p < 0 || (size_t)p >= order.size() || seen[(size_t)p]) return false;
        seen[(size_t)p] = 1;
    }
    return true;
}

// every slot's candidates (ordinals slot, slot + grid, ...) share w = p / S
static bool shares_warp(const std::vector<int> &order, int S, int grid)
{
    for (int slot = 0; slot < grid && (size_t)slot < order.size(); ++slot)
        for (size_t o = (size_t)slot + (size_t)grid; o < order.size(); o += (size_t)grid)
            if (order[o] / S != order[(size_t)slot] / S) return false;
    return true;
}

// images (warps + renders) the 32 or so workgroups of one XCD touch in one round, at most
static int xcd_images(const std::vector<int> &order, int S, int Wn, int grid)
{
    int worst = 0;
    for (size_t round = 0; round * (size_t)grid < order.size(); ++round)
        for (int x = 0; x < 8; ++x) {
            std::vector<char> ws((size_t)Wn, 0), ss((size_t)S, 0);
            int n = 0;
            for (int b = x; b < grid; b += 8) {
                const int slot = (grid & 7) == 0 ? (b & 7) * (grid >> 3) + (b >> 3) : b;  // slot_in_round
                const size_t o = round * (size_t)grid + (size_t)slot;
                if (o >= order.size()) continue;
                const int w = order[o] / S, s = order[o] % S;
                n += !ws[(size_t)w] + !ss[(size_t)s];
                ws[(size_t)w] = ss[(size_t)s] = 1;
            }
            if (n > worst) worst = n;
        }
    return worst;
}

int main()
{
    static const int kGrids[] = {1, 8, 64, 243, 248, 256, 304};
    int shared = 0;
    for (int S = 1; S <= 40; ++S)
        for (int Wn = 1; Wn <= 40; ++Wn)
            for (int grid : kGrids) {
                const std::vector<int> order = order_of(S, Wn, grid);
                CHECK(is_permutation(order), "%d x %d on %d: not a permutation", S, Wn, grid);
                std::vector<int> t((size_t)S * Wn), probe((size_t)S * Wn, -1);
                tiles(S, Wn, t);
                if (nmi::build_shared_order(S, Wn, grid, probe.data())) {
                    ++shared;
                    CHECK(shares_warp(order, S, grid), "%d x %d on %d: a workgroup meets two warps", S, Wn, grid);
                } else {
                    CHECK(order == t, "%d x %d on %d: the fallback is not the tile order", S, Wn, grid);
                    for (int p : probe) CHECK(p == -1, "%d x %d on %d: a refused order was written to", S, Wn, grid);
                }
            }
    CHECK(shared > 500, "only %d shapes share", shared);

    // the shapes that must share
    static const int kShare[][3] = {{27, 27, 243}, {27, 27, 256}, {64, 64, 256}, {27, 27, 81}, {9, 27, 243}, {40, 40, 80}, {27, 4, 8}, {30, 30, 304}};
    for (const auto &c : kShare) {
        const std::vector<int> order = order_of(c[0], c[1], c[2]);
        CHECK(is_permutation(order) && shares_warp(order, c[0], c[2]), "%d x %d on %d does not share", c[0], c[1], c[2]);
    }
    // ... and what an XCD's round touches there: the tiles hold 12 images
    CHECK(xcd_images(order_of(27, 27, 243), 27, 27, 243) <= 14, "27 x 27 on 243: %d images", xcd_images(order_of(27, 27, 243), 27, 27, 243));
    CHECK(xcd_images(order_of(27, 27, 256), 27, 27, 256) <= 14, "27 x 27 on 256: %d images", xcd_images(order_of(27, 27, 256), 27, 27, 256));
    CHECK(xcd_images(order_of(64, 64, 256), 64, 64, 256) <= 12, "64 x 64 on 256: %d images", xcd_images(order_of(64, 64, 256), 64, 64, 256));
    printf("images per XCD round: 27x27/243 %d, 27x27/256 %d, 64x64/256 %d\n", xcd_images(order_of(27, 27, 243), 27, 27, 243),
           xcd_images(order_of(27, 27, 256), 27, 27, 256), xcd_images(order_of(64, 64, 256), 64, 64, 256));

    // the shapes that cannot: one round only, one render, one warp, S out of reach of R and R - 1 candidates per workgroup
    static const int kFallback[][3] = {{27, 27, 729}, {5, 7, 35}, {5, 7, 256}, {1, 9, 8}, {9, 1, 8}, {1, 300, 256}, {300, 1, 256},
                                       {5, 7, 8}, {3, 3, 2}, {7, 40, 64}, {40, 40, 64}};
    for (const auto &c : kFallback) {
        std::vector<int> t((size_t)c[0] * c[1]);
        tiles(c[0], c[1], t);
        CHECK(order_of(c[0], c[1], c[2]) == t, "%d x %d on %d: not the tile order", c[0], c[1], c[2]);
    }

    // the plan asks for the shared order for nmi_grid_kernel's own plain launches only
    nmi::PlanInputs in;
    in.compute_units = 256;
    in.total = 729;
    in.width = 640;
    in.npix = 640 * 480;
    in.vec_ok = true;
    in.split_checked = true;
    nmi::SearchPlan plan = nmi::plan_search(in);
    CHECK(plan.kind == nmi::SearchKernel::grid && plan.order_table && plan.shared_order && plan.workgroups == 256, "plain 27 x 27");
    in.few_hint = true;
    plan = nmi::plan_search(in);
    CHECK(plan.kind == nmi::SearchKernel::few_levels && plan.order_table && !plan.shared_order, "few levels");
    in.few_hint = false;
    in.xcd_tiling = false;
    plan = nmi::plan_search(in);
    CHECK(!plan.order_table && !plan.shared_order, "no table");
    in.xcd_tiling = true;
    for (nmi::SearchForm f : {nmi::SearchForm::masked, nmi::SearchForm::level}) {
        in.form = f;
        plan = nmi::plan_search(in);
        CHECK(plan.order_table && !plan.shared_order, "masked and level searches keep the tiles");
    }
    in.form = nmi::SearchForm::plain;
    in.total = 100;  // pixel-range kernel
    plan = nmi::plan_search(in);
    CHECK(plan.kind == nmi::SearchKernel::pix && !plan.shared_order, "pixel ranges");

    if (failures) return 1;
    printf("search order ok\n");
    return 0;
}
