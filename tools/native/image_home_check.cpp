// Stand-alone host check of jxlatte_amd/csrc/image_home.h (no device, no context), meant for an AddressSanitizer + UBSan build
// (tests/test_image_home_cpu.py). It walks a matrix of homes -- host planes, resident planes of 5 x 7, and sets: an unknown one,
// five planes (float, float, float, int32, float), three (int32, float, int32) and one float plane, asked for 0 .. 4 colour planes
// and the alpha planes -2, -1, 3, n - 1, n with and without has_alpha -- and of parameters: 5 x 7, 7 x 5, 5 x 8, four sets of
// colour tags, both alpha tags. One line per case, for the test to compare with its own statement of the rules:
//   CASE <kind> <view> <n_color> <alpha_plane> <has_alpha> <height> <width> <tag0><tag1><tag2> <alpha tag> : <first half>
//        <second half> <colour planes to upload> <alpha plane to upload>
// Beside the codes it checks here what a home hands on: the planes' pointers and tags. Ends with "<n> failure(s)".
#include <cstdio>

#include "../../jxlatte_amd/csrc/image_home.h"

using namespace jxl;

static int failures = 0;
#define EXPECT(cond, what)                          \
    do {                                            \
        if (!(cond)) {                              \
            printf("FAIL: %s (%s)\n", what, #cond); \
            failures++;                             \
        }                                           \
    } while (0)

static uint32_t g_planes[5][35];
static const int kViewN[3] = {5, 3, 1};
static const int kViewTypes[3][5] = {{0, 0, 0, 1, 0}, {1, 0, 1, 0, 0}, {0, 0, 0, 0, 0}};

static CanvasView view(int which) {
    CanvasView v{};
    v.n = kViewN[which], v.h = 5, v.w = 7;
    for (int i = 0; i < v.n; i++) v.type[i] = kViewTypes[which][i] ? JXL_PLANE_INT32 : JXL_PLANE_FLOAT, v.plane[i] = g_planes[i];
    return v;
}

// the second half of `m` under every set of parameters, one line each
static void describe(const ImageHome& m, int which, int n_color, int alpha_plane, int has_alpha) {
    static const int sizes[3][2] = {{5, 7}, {7, 5}, {5, 8}};
    static const int32_t tags[4][3] = {{0, 0, 0}, {1, 1, 1}, {1, 0, 0}, {1, 0, 1}};
    const HomeUploads up = home_uploads(m);
    for (const auto& s : sizes)
        for (const auto& t : tags)
            for (int at = 0; at < 2; at++) {
                const HomeRefusal r = home_describes(m, s[0], s[1], n_color, t, at);
                if (t[0] == t[1] && t[1] == t[2]) EXPECT(r == home_describes(m, s[0], s[1], n_color, t[0], at), "one tag for every colour plane");
                printf("CASE %d %d %d %d %d %d %d %d%d%d %d : %d %d %d %d\n", (int)m.kind, which, n_color, alpha_plane, has_alpha, s[0], s[1],
                       (int)t[0], (int)t[1], (int)t[2], at, (int)m.planes, (int)r, (int)up.color, (int)up.alpha);
            }
}

int main() {
    const void* in[3] = {g_planes[0], g_planes[1], g_planes[2]};
    const void* alpha = g_planes[3];

    ImageHome m = home_host(in, alpha);
    EXPECT(m.kind == HOME_HOST && m.planes == HOME_OK && m.in() == m.color && m.color[2] == in[2] && m.alpha == alpha && !m.alpha_on_device, "host planes");
    for (int n = 1; n <= 3; n += 2) describe(m, -1, n, -1, 1);
    m = home_host(nullptr, nullptr);
    EXPECT(m.in() == nullptr && !m.alpha && home_describes(m, 5, 7, 3, 0, 0) == HOME_OK, "a null array is the argument checks' to refuse");
    in[1] = nullptr;
    EXPECT(home_host(in, nullptr).in() != nullptr && !home_host(in, nullptr).color[1], "a null plane too");
    in[1] = g_planes[1];

    m = home_resident(5, 7, in, alpha);
    EXPECT(m.kind == HOME_RESIDENT && m.planes == HOME_OK && m.h == 5 && m.w == 7 && m.n == 3 && m.in() == m.color && m.color[1] == in[1], "resident planes");
    EXPECT(m.alpha == alpha && !m.alpha_on_device && !m.color_int[0] && !m.color_int[1] && !m.color_int[2], "resident planes: float, alpha from the host");
    for (int n = 1; n <= 3; n += 2) describe(m, -1, n, -1, 1);

    for (int which = -1; which < 3; which++) {
        const CanvasView v = which < 0 ? CanvasView{} : view(which);
        const int n = which < 0 ? 5 : v.n;
        const int alphas[5] = {-2, -1, 3, n - 1, n};
        for (int n_color = 0; n_color <= 4; n_color++)
            for (int alpha_plane : alphas)
                for (int has_alpha = 0; has_alpha < 2; has_alpha++) {
                    m = home_set(which < 0 ? nullptr : &v, n_color, alpha_plane, has_alpha != 0);
                    EXPECT(m.kind == HOME_SET && m.alpha_on_device && m.in() == m.color, "a set");
                    if (m.planes == HOME_OK) {
                        EXPECT(m.h == 5 && m.w == 7 && m.n == v.n, "a set's geometry");
                        for (int i = 0; i < 3; i++)
                            EXPECT(m.color[i] == (i < n_color ? (const void*)v.plane[i] : nullptr), "a set's colour planes, null behind them");
                        for (int i = 0; i < n_color; i++) EXPECT(m.color_int[i] == (v.type[i] == JXL_PLANE_INT32), "a set's colour tags");
                        EXPECT(m.alpha == (alpha_plane >= 0 ? (const void*)v.plane[alpha_plane] : nullptr), "a set's alpha plane");
                        if (alpha_plane >= 0) EXPECT(m.alpha_int == (v.type[alpha_plane] == JXL_PLANE_INT32), "a set's alpha tag");
                    } else {
                        EXPECT(!m.color[0] && !m.color[1] && !m.color[2] && !m.alpha, "a refused set hands on no plane");
                    }
                    describe(m, which, n_color, alpha_plane, has_alpha);
                }
    }
    printf("%d failure(s)\n", failures);
    return failures ? 1 : 0;
}
