// Stand-alone host check of jxlatte_amd/csrc/tensor_resize_check.h (no device, no context), meant for an AddressSanitizer +
// UBSan build (tests/test_tensor_resized_cpu.py): the box, size and filter rules, the tap-table builder, the cap of 1024 taps,
// the tile picker and the rule of the 16-byte plane loads, over a table of cases. Then, for every "L O filter" triple on the
// command line, the axis' table as the kernel gets it:
//   TAPS <L> <O> <filter> <n>        and per output   T <first> <count> <weight bits, hex> ...
// Ends with "<n> failure(s)".
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../jxlatte_amd/csrc/tensor_resize_check.h"

static int failures = 0;
#define EXPECT(cond, what)                          \
    do {                                            \
        if (!(cond)) {                              \
            printf("FAIL: %s (%s)\n", what, #cond); \
            failures++;                             \
        }                                           \
    } while (0)

static jxl_tensor_params tensor(int h, int w) {
    jxl_tensor_params p;
    memset(&p, 0, sizeof p);
    p.color.n_planes = 3;
    p.height = h, p.width = w;
    p.dtype = JXL_TENSOR_F32, p.layout = JXL_TENSOR_CHW;
    p.alpha_tagged_depth = p.color_tagged_depth = 8;
    return p;
}

static jxl_resize_params whole(int h, int w, int oh, int ow, int filter = JXL_RESIZE_TRIANGLE) {
    jxl_resize_params r = {0, 0, w, h, oh, ow, filter};
    return r;
}

static void params() {
    const jxl_tensor_params p = tensor(33, 67);
    jxl_resize_params r = whole(33, 67, 8, 5);
    EXPECT(jxl::resize_check_params(&p, &r) == nullptr, "the whole image");
    EXPECT(jxl::resize_check_params(nullptr, &r) && jxl::resize_check_params(&p, nullptr), "null arguments");
    r.filter = 2;
    EXPECT(jxl::resize_check_params(&p, &r), "unknown filter");
    r.filter = -1;
    EXPECT(jxl::resize_check_params(&p, &r), "negative filter");
    r = whole(33, 67, 0, 5);
    EXPECT(jxl::resize_check_params(&p, &r), "out height 0");
    r = whole(33, 67, 8, -1);
    EXPECT(jxl::resize_check_params(&p, &r), "out width < 0");
    const int boxes[][4] = {{-1, 0, 4, 4}, {0, -1, 4, 4}, {0, 0, 0, 4}, {0, 0, 4, 0}, {64, 0, 4, 4}, {0, 30, 4, 4}, {67, 0, 1, 1},
                            {1, 0, INT32_MAX, 4}, {0, 1, 4, INT32_MAX}, {INT32_MAX, INT32_MAX, INT32_MAX, INT32_MAX}};
    for (const auto& b : boxes) {
        r = whole(33, 67, 8, 5);
        r.box_x0 = b[0], r.box_y0 = b[1], r.box_width = b[2], r.box_height = b[3];
        EXPECT(jxl::resize_check_params(&p, &r), "a box outside the image, empty, or past 2^31");
    }
    r = whole(33, 67, 6, 4);
    r.box_x0 = 3, r.box_y0 = 2, r.box_width = 20, r.box_height = 9;
    EXPECT(jxl::resize_check_params(&p, &r) == nullptr, "a box inside");
    r.box_x0 = 47, r.box_y0 = 24;
    EXPECT(jxl::resize_check_params(&p, &r) == nullptr, "a box that ends with the image");
    jxl_tensor_params q = tensor(0, 67);
    r = whole(33, 67, 8, 5);
    EXPECT(jxl::resize_check_params(&q, &r), "a source of no rows");
}

static void taps() {
    jxl::ResizeTaps t;
    for (int filter = 0; filter < 2; filter++) {
        EXPECT(jxl::resize_build_taps(67, 67, filter, &t) == nullptr && t.w.size() == 67, "identity: one tap each");
        bool one = true;
        for (int o = 0; o < 67; o++) one = one && t.first[o] == o && t.off[o + 1] == o + 1 && t.w[o] == 1.0f;
        EXPECT(one, "identity: first = o, weight 1");
        EXPECT(jxl::resize_build_taps(1, 3, filter, &t) == nullptr && t.w.size() == 3 && t.first[2] == 0, "upscaling from one sample");
        EXPECT(jxl::resize_build_taps(0, 3, filter, &t) && jxl::resize_build_taps(3, 0, filter, &t), "empty axes");
        EXPECT(jxl::resize_build_taps((int64_t)INT32_MAX + 1, 3, filter, &t), "an axis past 2^31");
    }
    EXPECT(jxl::resize_build_taps(2100, 5, JXL_RESIZE_TRIANGLE, &t) == nullptr, "840 taps");
    int widest = 0;
    for (int o = 0; o < 5; o++) widest = t.off[o + 1] - t.off[o] > widest ? t.off[o + 1] - t.off[o] : widest;
    EXPECT(widest > 800 && widest <= 841, "840 taps: the widest range");
    EXPECT(jxl::resize_build_taps(2100, 3, JXL_RESIZE_TRIANGLE, &t), "1400 taps: refused");
    EXPECT(jxl::resize_build_taps(2100, 3, JXL_RESIZE_BOX, &t) == nullptr, "700 taps of the box");
    EXPECT(jxl::resize_build_taps(2100, 2, JXL_RESIZE_BOX, &t), "1050 taps of the box: refused");
    EXPECT(jxl::resize_build_taps(INT32_MAX, 1, JXL_RESIZE_BOX, &t), "2^31 taps: refused before anything of that size is made");
    // every range inside [0, L), weights summing to 1 within the f32 roundings
    const int pairs[][2] = {{1, 1}, {7, 3}, {7, 11}, {67, 5}, {33, 8}, {48, 3}, {64, 4}, {20, 4}, {9, 6}, {3840, 224}, {2160, 224}, {1000, 999}};
    for (const auto& pr : pairs)
        for (int filter = 0; filter < 2; filter++) {
            EXPECT(jxl::resize_build_taps(pr[0], pr[1], filter, &t) == nullptr, "a table");
            bool in = true, unit = true;
            for (int o = 0; o < pr[1]; o++) {
                const int n = t.off[o + 1] - t.off[o];
                in = in && n >= 1 && t.first[o] >= 0 && t.first[o] + n <= pr[0];
                double sum = 0;
                for (int k = 0; k < n; k++) sum += t.w[t.off[o] + k];
                unit = unit && sum > 1 - 1e-4 && sum < 1 + 1e-4;
            }
            EXPECT(in && unit, "ranges inside the axis, weights of sum 1");
        }
}

static void tiles() {
    jxl::ResizeTaps x, y;
    jxl::ResizeTile t;
    EXPECT(jxl::resize_build_taps(3840, 224, JXL_RESIZE_TRIANGLE, &x) == nullptr, "3840 -> 224");
    EXPECT(jxl::resize_build_taps(2160, 224, JXL_RESIZE_TRIANGLE, &y) == nullptr, "2160 -> 224");
    EXPECT(jxl::resize_band_rows(y, 1) >= 19 && jxl::resize_band_rows(y, 1) <= 21 && jxl::resize_band_rows(y, 4) >= 48 && jxl::resize_band_rows(y, 4) <= 50, "rows of a band");
    // 512 slots: 32 x 4 is one round of 392 tiles, one chunk, 49 rows; 64 x 4 needs two chunks, 64 x 2 walks 2 x 30 rows
    EXPECT(jxl::resize_pick_tile(x, 0, y, 3, true, 512, 0, 0, &t) == nullptr && t.tw == 32 && t.th == 4 && t.lds_bytes <= jxl::kResizeLdsBytes, "the headline tile");
    EXPECT(t.lds_bytes == t.th * 3 * t.lds_w * 4, "the LDS image's size");
    EXPECT(jxl::resize_pick_tile(x, 0, y, 3, true, 0, 0, 0, &t) == nullptr && t.lds_bytes <= jxl::kResizeLdsBytes, "no slot count: still a tile");
    EXPECT(jxl::resize_pick_tile(x, 0, y, 3, true, 512, 16, 2, &t) == nullptr && t.tw == 16 && t.th == 2, "a forced tile");
    EXPECT(jxl::resize_pick_tile(x, 0, y, 3, true, 512, 24, 2, &t) && jxl::resize_pick_tile(x, 0, y, 3, true, 512, 16, 3, &t) && jxl::resize_pick_tile(x, 0, y, 3, true, 512, 0, 2, &t),
           "tiles the kernel does not have");
    EXPECT(jxl::resize_build_taps(7, 3, JXL_RESIZE_BOX, &y) == nullptr, "a short y axis");
    // at the cap every filter and plane count launches: the narrowest tile fits
    EXPECT(jxl::resize_build_taps(1024 * 8, 16, JXL_RESIZE_TRIANGLE, &x) == nullptr, "1024 taps of the triangle");
    EXPECT(jxl::resize_pick_tile(x, 3, y, 4, true, 512, 0, 0, &t) == nullptr && t.lds_bytes <= jxl::kResizeLdsBytes, "a tile at the cap, four planes");
    EXPECT(jxl::resize_pick_tile(x, 3, y, 4, true, 512, 64, 4, &t), "the widest tile does not fit there: refused, not launched");
    EXPECT(jxl::resize_build_taps(1024 * 16, 16, JXL_RESIZE_BOX, &x) == nullptr, "1024 taps of the box");
    EXPECT(jxl::resize_pick_tile(x, 1, y, 4, true, 512, 0, 0, &t) == nullptr && t.lds_bytes <= jxl::kResizeLdsBytes, "a tile at the box's cap");
    EXPECT(jxl::resize_lds_col(0, true) == 0 && jxl::resize_lds_col(31, true) == 31 && jxl::resize_lds_col(32, true) == 33 && jxl::resize_lds_col(32, false) == 32, "the skew");
    const uint64_t al[3] = {0x1000, 0x2000, 0x3010}, un[2] = {0x1000, 0x2004};
    EXPECT(jxl::resize_wide_in_ok(64, al, 3) && !jxl::resize_wide_in_ok(66, al, 3) && !jxl::resize_wide_in_ok(64, un, 2) && jxl::resize_wide_in_ok(64, un, 1), "16-byte loads");
}

int main(int argc, char** argv) {
    params();
    taps();
    tiles();
    for (int i = 1; i + 2 < argc; i += 3) {
        const long L = atol(argv[i]), O = atol(argv[i + 1]);
        const int filter = atoi(argv[i + 2]);
        jxl::ResizeTaps t;
        const char* why = jxl::resize_build_taps(L, O, filter, &t);
        if (why) {
            printf("TAPS %ld %ld %d refused: %s\n", L, O, filter, why);
            continue;
        }
        printf("TAPS %ld %ld %d %zu\n", L, O, filter, t.w.size());
        for (long o = 0; o < O; o++) {
            printf("T %d %d", t.first[o], t.off[o + 1] - t.off[o]);
            for (int k = t.off[o]; k < t.off[o + 1]; k++) {
                uint32_t bits;
                memcpy(&bits, &t.w[k], 4);
                printf(" %08x", bits);
            }
            printf("\n");
        }
    }
    printf("%d failure(s)\n", failures);
    return failures ? 1 : 0;
}
