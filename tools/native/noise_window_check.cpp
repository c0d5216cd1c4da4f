// Stand-alone host check of jxlatte_amd/csrc/noise_window_check.h (no device, no context), meant for an AddressSanitizer + UBSan
// build (tests/test_region_cpu.py). For every accepted argument set the two launches of k_noise_window.hip are replayed on the
// host as index arithmetic over allocations of exactly the plan's sizes:
//   * the generator's stores: every sample of the apron is stored exactly once, by the group that holds it, and nothing else is;
//   * the convolution's loads: noise_mirror of every coordinate it forms lies inside the apron (no clamp here: a miss is a read
//     outside the allocation, which the sanitizer reports, and a FAIL line).
// Then the refusals. Then, for every "group_dim frame_h frame_w y0 x0 win_h win_w" on the command line, the plan:
//   PLAN <ay0> <ax0> <ah> <aw> <gy0> <gx0> <gh> <gw> <n_groups> <apron_floats> <window_floats>      or      REFUSED <why>
// Ends with "<n> failure(s)".
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../jxlatte_amd/csrc/noise_window_check.h"

using namespace jxl;

static int failures = 0;
#define EXPECT(cond, what)                          \
    do {                                            \
        if (!(cond)) {                              \
            printf("FAIL: %s (%s)\n", what, #cond); \
            failures++;                             \
        }                                           \
    } while (0)

static const float kLut[8] = {0, 0.1f, 0.2f, 0.3f, 0.4f, 0.5f, 0.6f, 0.7f};

// the index arithmetic of k_noise_window_rng and k_noise_window_add, without the samples
static void replay(const NoiseWindowPlan& p, const char* what) {
    std::vector<uint8_t> apron((size_t)p.apron_floats, 0);  // per sample: how often it was stored
    const int gd = p.group_dim, ay1 = p.ay0 + p.ah, ax1 = p.ax0 + p.aw;
    for (int group = 0; group < p.n_groups; group++) {
        const int y0 = (p.gy0 + group / p.gw) * gd, x0 = (p.gx0 + group % p.gw) * gd;
        EXPECT(y0 < p.frame_h && x0 < p.frame_w, what);
        const int ySize = gd < p.frame_h - y0 ? gd : p.frame_h - y0, xSize = gd < p.frame_w - x0 ? gd : p.frame_w - x0;
        for (int y = 0; y < ySize; y++) {
            const int Y = y0 + y;
            if (Y < p.ay0 || Y >= ay1) continue;
            const int64_t row = (int64_t)(Y - p.ay0) * p.aw - p.ax0;
            for (int x = 0; x < xSize; x += 16)
                for (int lane = 0; lane < 8; lane++)
                    for (int k = 0; k < 2; k++) {
                        const int px = x + 2 * lane + k, X = x0 + px;
                        if (px < xSize && X >= p.ax0 && X < ax1) apron[(size_t)(row + X)]++;
                    }
        }
    }
    bool once = true;
    for (uint8_t n : apron) once &= n == 1;
    EXPECT(once, what);
    std::vector<uint8_t> window((size_t)p.window_floats, 0);
    int64_t sum = 0;
    for (int64_t i = 0; i < p.window_floats; i++) {
        const int wy = (int)(i / p.win_w), wx = (int)(i - (int64_t)wy * p.win_w);
        for (int iy = 0; iy < 5; iy++)
            for (int ix = 0; ix < 5; ix++) {
                const int cy = noise_mirror(p.y0 + wy + iy - 2, p.frame_h) - p.ay0, cx = noise_mirror(p.x0 + wx + ix - 2, p.frame_w) - p.ax0;
                if (cy < 0 || cy >= p.ah || cx < 0 || cx >= p.aw) {
                    EXPECT(false, what);
                    continue;
                }
                sum += apron[(size_t)((int64_t)cy * p.aw + cx)];
            }
        window[(size_t)i]++;
    }
    EXPECT(sum == 25 * p.window_floats, what);
    EXPECT(noise_window_apron_holds(p), what);
}

static bool accept(int gd, int fh, int fw, int y0, int x0, int wh, int ww, NoiseWindowPlan* p) {
    return noise_window_check(gd, kLut, fh, fw, y0, x0, wh, ww, p) == nullptr;
}

int main(int argc, char** argv) {
    NoiseWindowPlan p;
    // the windows of the device tests, (x0, y0, w, h) on a frame 520 wide and 264 high, of 256-pixel groups
    static const int kWin[][4] = {{0, 0, 20, 20}, {250, 0, 12, 264}, {500, 244, 20, 20}, {255, 255, 2, 2}, {0, 0, 520, 264}, {519, 263, 1, 1}};
    for (const auto& w : kWin) {
        EXPECT(accept(256, 264, 520, w[1], w[0], w[3], w[2], &p), "a window of the device tests");
        replay(p, "a window of the device tests");
    }
    // every window of small frames, tiny ones included (the mirror bounces more than once there), with 16-pixel groups
    for (int fh = 1; fh <= 6; fh++)
        for (int fw = 1; fw <= 6; fw++)
            for (int y0 = 0; y0 < fh; y0++)
                for (int x0 = 0; x0 < fw; x0++)
                    for (int wh = 1; y0 + wh <= fh; wh++)
                        for (int ww = 1; x0 + ww <= fw; ww++) {
                            EXPECT(accept(16, fh, fw, y0, x0, wh, ww, &p), "a window of a tiny frame");
                            replay(p, "a window of a tiny frame");
                        }
    // windows around group corners and frame edges of a 3 x 3 grid of 16-pixel groups whose last row and column are ragged
    for (int y0 : {0, 1, 2, 13, 14, 15, 16, 17, 18, 30, 33, 36})
        for (int x0 : {0, 2, 14, 15, 16, 18, 31, 32, 34, 38})
            for (int wh : {1, 2, 3, 17})
                for (int ww : {1, 4, 16, 33}) {
                    if (y0 + wh > 37 || x0 + ww > 39) continue;
                    EXPECT(accept(16, 37, 39, y0, x0, wh, ww, &p), "a window around a group corner");
                    replay(p, "a window around a group corner");
                    EXPECT(p.gh >= 1 && p.gw >= 1 && p.gy0 + p.gh <= 3 && p.gx0 + p.gw <= 3, "the groups lie in the frame's grid");
                }
    // sizes: the largest frame, counted in 64 bits (not replayed)
    EXPECT(accept(256, 32768, 32768, 0, 0, 32768, 32768, &p) && p.window_floats == (int64_t)1 << 30 && p.apron_floats == (int64_t)1 << 30 &&
               p.n_groups == 128 * 128, "the largest frame");
    EXPECT(accept(256, 1, 1 << 30, 0, (1 << 30) - 1, 1, 1, &p) && p.aw == 3 && p.n_groups == 1, "a one-row frame of 2^30 columns");
    // refusals
    EXPECT(!accept(256, 32768, 32769, 0, 0, 1, 1, &p), "a frame of more than 2^30 pixels");
    EXPECT(!accept(256, 0, 8, 0, 0, 1, 1, &p) && !accept(256, 8, -1, 0, 0, 1, 1, &p), "an empty frame");
    EXPECT(!accept(256, 8, 8, 0, 0, 0, 1, &p) && !accept(256, 8, 8, 0, 0, 1, -3, &p), "an empty window");
    EXPECT(!accept(256, 8, 8, -1, 0, 1, 1, &p) && !accept(256, 8, 8, 0, -1, 1, 1, &p), "a negative origin");
    EXPECT(!accept(256, 8, 8, 0, 0, 9, 1, &p) && !accept(256, 8, 8, 4, 4, 4, 5, &p), "a window that leaves the frame");
    EXPECT(!accept(256, 8, 8, 2147483647, 0, 2, 1, &p) && !accept(256, 8, 8, 0, 2147483647, 1, 2147483647, &p), "a window whose end overflows 32 bits");
    EXPECT(!accept(8, 8, 8, 0, 0, 1, 1, &p) && !accept(24, 8, 8, 0, 0, 1, 1, &p) && !accept(0, 8, 8, 0, 0, 1, 1, &p) &&
               !accept(-256, 8, 8, 0, 0, 1, 1, &p) && !accept(1 << 17, 8, 8, 0, 0, 1, 1, &p), "a bad group size");
    EXPECT(noise_window_check(256, nullptr, 8, 8, 0, 0, 1, 1, &p) != nullptr && noise_window_check(256, kLut, 8, 8, 0, 0, 1, 1, nullptr) != nullptr,
           "a null argument");
    for (int i = 1; i + 6 < argc; i += 7) {
        int v[7];
        for (int k = 0; k < 7; k++) v[k] = atoi(argv[i + k]);
        const char* why = noise_window_check(v[0], kLut, v[1], v[2], v[3], v[4], v[5], v[6], &p);
        if (why) {
            printf("REFUSED %s\n", why);
            continue;
        }
        replay(p, "a window of the command line");
        printf("PLAN %d %d %d %d %d %d %d %d %d %" PRId64 " %" PRId64 "\n", p.ay0, p.ax0, p.ah, p.aw, p.gy0, p.gx0, p.gh, p.gw, p.n_groups,
               p.apron_floats, p.window_floats);
    }
    printf("%d failure(s)\n", failures);
    return failures ? 1 : 0;
}
