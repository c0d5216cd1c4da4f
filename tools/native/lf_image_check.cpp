// Stand-alone host check of jxlatte_amd/csrc/lf_image_check.h (no device, no context), meant for an AddressSanitizer + UBSan
// build (tests/test_lf_preview_cpu.py): descriptors the validator accepts -- with the plan it makes of them, every integer the
// plan names read -- and the ones it refuses. Then, for every "cells_h cells_w" pair on the command line, the plan of a descriptor
// of that size with its groups in reverse order:
//   PLAN <grows> <gcols> <total_ints> <order[0]> ... <q_off[0]> ...
// Ends with "<n> failure(s)".
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../jxlatte_amd/csrc/lf_image_check.h"

static int failures = 0;
#define EXPECT(cond, what)                          \
    do {                                            \
        if (!(cond)) {                              \
            printf("FAIL: %s (%s)\n", what, #cond); \
            failures++;                             \
        }                                           \
    } while (0)

// a descriptor of cells_h x cells_w whose groups tile the grid, in reverse raster order, each plane an allocation of exactly its size
struct Desc {
    jxl_lf_image_desc d;
    std::vector<jxl_lfquant_desc> groups;
    std::vector<std::vector<int32_t>> planes;
    std::vector<float> out[3];
    const float* outp[3];
    Desc(int ch, int cw) {
        memset(&d, 0, sizeof d);
        const int gr = (ch + 255) / 256, gc = (cw + 255) / 256;
        for (int p = gr * gc - 1; p >= 0; p--) {
            jxl_lfquant_desc g;
            memset(&g, 0, sizeof g);
            g.lfg_y = p / gc, g.lfg_x = p % gc;
            g.cells_h = ch - g.lfg_y * 256 < 256 ? ch - g.lfg_y * 256 : 256;
            g.cells_w = cw - g.lfg_x * 256 < 256 ? cw - g.lfg_x * 256 : 256;
            g.extra_precision = p & 3;
            groups.push_back(g);
        }
        planes.resize(groups.size() * 3);
        for (size_t i = 0; i < groups.size(); i++)
            for (int c = 0; c < 3; c++) {
                planes[i * 3 + c].assign((size_t)groups[i].cells_h * groups[i].cells_w, (int32_t)(i * 3 + c + 1));
                groups[i].lf_quant[c] = planes[i * 3 + c].data();
            }
        d.n_groups = (int32_t)groups.size();
        d.cells_h = ch, d.cells_w = cw;
        d.color_factor = 84;
        d.groups = groups.data();
        for (int c = 0; c < 3; c++) {
            out[c].assign((size_t)ch * cw, 0.0f);
            outp[c] = out[c].data();
        }
    }
};

// the plan of an accepted descriptor: every position has its group, the offsets are the prefix sums of the groups' planes in grid
// order, and what the host entry copies -- cells_h * cells_w ints from each plane to its offset -- stays inside a block of total_ints
static void accepted(int ch, int cw, bool print) {
    Desc t(ch, cw);
    jxl::LfImagePlan plan;
    const char* why = jxl::lf_image_check(&t.d, t.outp, true, &plan);
    EXPECT(why == nullptr, "a tiling descriptor is accepted");
    if (why) return;
    EXPECT(jxl::lf_image_check(&t.d, nullptr, false, &plan) == nullptr, "and without host planes where none are asked for");
    EXPECT(plan.grows * plan.gcols == t.d.n_groups && plan.total_ints == (int64_t)3 * ch * cw, "grid and total");
    std::vector<int32_t> block((size_t)plan.total_ints, 0);
    int64_t at = 0;
    for (int p = 0; p < t.d.n_groups; p++) {
        const jxl_lfquant_desc& g = t.d.groups[plan.order[(size_t)p]];
        EXPECT(g.lfg_y == p / plan.gcols && g.lfg_x == p % plan.gcols, "order[] leads to the group of the position");
        for (int c = 0; c < 3; c++) {
            EXPECT(plan.q_off[(size_t)p * 3 + c] == at, "offsets are prefix sums");
            const size_t n = (size_t)g.cells_h * g.cells_w;
            memcpy(block.data() + plan.q_off[(size_t)p * 3 + c], g.lf_quant[c], 4 * n);  // (the host entry's copy)
            at += (int64_t)n;
        }
    }
    if (print) {
        printf("PLAN %d %d %" PRId64, plan.grows, plan.gcols, plan.total_ints);
        for (int v : plan.order) printf(" %d", v);
        for (int64_t v : plan.q_off) printf(" %" PRId64, v);
        printf("\n");
    }
}

static void refusals() {
    jxl::LfImagePlan plan;
    {
        Desc t(33, 288);
        EXPECT(jxl::lf_image_check(nullptr, t.outp, true, &plan), "null descriptor");
        EXPECT(jxl::lf_image_check(&t.d, nullptr, true, &plan), "null output array");
        const float* two[3] = {t.outp[0], nullptr, t.outp[2]};
        EXPECT(jxl::lf_image_check(&t.d, two, true, &plan), "a null output plane");
        t.d.groups = nullptr;
        EXPECT(jxl::lf_image_check(&t.d, t.outp, true, &plan), "null group array");
    }
    {
        Desc t(33, 288);
        t.d.color_factor = 0;
        EXPECT(jxl::lf_image_check(&t.d, t.outp, true, &plan), "color_factor == 0");
    }
    {
        Desc t(33, 288);
        t.groups[0].lfg_x = t.groups[1].lfg_x;  // both at (0, 0): an overlap, and (0, 1) stays empty
        t.groups[0].cells_w = t.groups[1].cells_w;
        EXPECT(jxl::lf_image_check(&t.d, t.outp, true, &plan), "two groups at one position");
    }
    {
        Desc t(33, 288);
        t.groups[0].lfg_x = 2;
        EXPECT(jxl::lf_image_check(&t.d, t.outp, true, &plan), "a group outside the grid (x)");
        t.groups[0].lfg_x = 1, t.groups[0].lfg_y = 1;
        EXPECT(jxl::lf_image_check(&t.d, t.outp, true, &plan), "a group outside the grid (y)");
        t.groups[0].lfg_y = -1;
        EXPECT(jxl::lf_image_check(&t.d, t.outp, true, &plan), "a negative position");
    }
    {
        Desc t(33, 288);
        t.groups[1].cells_w = 257;
        EXPECT(jxl::lf_image_check(&t.d, t.outp, true, &plan), "a 257-cell group");
        t.groups[1].cells_w = 0;
        EXPECT(jxl::lf_image_check(&t.d, t.outp, true, &plan), "a group without cells");
        t.groups[1].cells_w = 255;
        EXPECT(jxl::lf_image_check(&t.d, t.outp, true, &plan), "a group smaller than its tile");
        t.groups[1].cells_w = 256, t.groups[0].cells_w = 33;
        EXPECT(jxl::lf_image_check(&t.d, t.outp, true, &plan), "a group larger than its tile");
    }
    {
        Desc t(33, 288);
        t.groups[1].lf_quant[2] = nullptr;
        EXPECT(jxl::lf_image_check(&t.d, t.outp, true, &plan), "a null LF plane");
    }
    {
        Desc t(33, 288);
        t.groups[0].extra_precision = 4;
        EXPECT(jxl::lf_image_check(&t.d, t.outp, true, &plan), "extra_precision 4");
        t.groups[0].extra_precision = -1;
        EXPECT(jxl::lf_image_check(&t.d, t.outp, true, &plan), "extra_precision -1");
    }
    {
        Desc t(33, 288);
        t.d.n_groups = 1;
        EXPECT(jxl::lf_image_check(&t.d, t.outp, true, &plan), "fewer groups than the grid has positions");
        t.d.n_groups = 3;  // (refused by the count: groups[2] is never read)
        EXPECT(jxl::lf_image_check(&t.d, t.outp, true, &plan), "more groups than the grid has positions");
        t.d.n_groups = 2, t.d.cells_h = 0;
        EXPECT(jxl::lf_image_check(&t.d, t.outp, true, &plan), "an empty output");
        t.d.cells_h = 1 << 20, t.d.cells_w = 1 << 20;
        EXPECT(jxl::lf_image_check(&t.d, t.outp, true, &plan), "an output beyond the cap (no product overflows)");
    }
}

int main(int argc, char** argv) {
    const int sizes[][2] = {{1, 1}, {2, 7}, {3, 3}, {33, 47}, {33, 288}, {257, 2}, {260, 300}, {256, 256}, {512, 257}};
    for (const auto& s : sizes) accepted(s[0], s[1], false);
    refusals();
    for (int i = 1; i + 1 < argc; i += 2) accepted(atoi(argv[i]), atoi(argv[i + 1]), true);
    printf("%d failure(s)\n", failures);
    return failures ? 1 : 0;
}
