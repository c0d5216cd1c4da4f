// Stand-alone host check of jxlatte_amd/csrc/tone_map_check.h and tone_map_ops.h (no device, no context), meant for an
// AddressSanitizer + UBSan build (tests/test_tone_map_cpu.py):
//   * the validator over a table of good and bad parameter blocks;
//   * the host-side constants of the good ones: finite, ordered, and the closed forms they must meet;
//   * the operator itself (the header is host-callable) over a few thousand seeded pixels: finite in, finite out; with the gamut
//     step every sample in [0, 1]; a grey pixel at the content's peak comes out at the display's.
// For every "unit source target gamut r g b" on the command line: "PIXEL <r> <g> <b>" (%.9g) of the operator, or "REFUSED <why>".
// Ends with "<n> failure(s)".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>

#include "../../jxlatte_amd/csrc/tone_map_check.h"

using namespace jxl;

static int failures = 0;
#define EXPECT(cond, what)                          \
    do {                                            \
        if (!(cond)) {                              \
            printf("FAIL: %s (%s)\n", what, #cond); \
            failures++;                             \
        }                                           \
    } while (0)

static const float kLum2020[3] = {0.2627f, 0.6780f, 0.0593f};

static jxl_tone_map block(float unit, float source, float target, int gamut, const float lum[3] = kLum2020) {
    jxl_tone_map t;
    for (int i = 0; i < 3; i++) t.lum[i] = lum[i];
    t.unit_nits = unit, t.source_nits = source, t.target_nits = target, t.gamut = gamut;
    return t;
}

static uint32_t rng_state = 0x1234567u;
static float rnd() {  // xorshift32 -> [0, 1)
    rng_state ^= rng_state << 13, rng_state ^= rng_state >> 17, rng_state ^= rng_state << 5;
    return (float)(rng_state >> 8) * (1.0f / 16777216.0f);
}

int main(int argc, char** argv) {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    // ---- the validator ----
    const jxl_tone_map good[] = {block(10000, 1000, 203, 1), block(10000, 10000, 203, 0), block(255, 255, 255, 1), block(4000, 4000, 100, 1),
                                 block(1, 0.5f, 1e-3f, 0), block(80, 80, 1000, 1)};
    for (const auto& t : good) EXPECT(tone_map_check(&t) == nullptr, "a good block");
    EXPECT(tone_map_check(nullptr) != nullptr, "a null block");
    for (float bad : {0.0f, -1.0f, inf, -inf, nan}) {
        jxl_tone_map t = block(bad, 1000, 203, 1);
        EXPECT(tone_map_check(&t) != nullptr, "bad unit_nits");
        t = block(10000, bad, 203, 1);
        EXPECT(tone_map_check(&t) != nullptr, "bad source_nits");
        t = block(10000, 1000, bad, 1);
        EXPECT(tone_map_check(&t) != nullptr, "bad target_nits");
    }
    {
        jxl_tone_map t = block(10000, 10000.001f * 1.001f, 203, 1);
        EXPECT(tone_map_check(&t) != nullptr, "source_nits above 10000");
        for (int g : {-1, 2, 255}) {
            t = block(10000, 1000, 203, g);
            EXPECT(tone_map_check(&t) != nullptr, "gamut other than 0 or 1");
        }
        const float w_nan[3] = {0.2f, nan, 0.1f}, w_inf[3] = {inf, 0.5f, 0.1f}, w_zero[3] = {0, 0, 0}, w_neg[3] = {-0.5f, 0.2f, 0.1f},
                    w_big[3] = {1.0f, 1.0f, 0.5f}, w_two[3] = {1.0f, 0.5f, 0.5f};
        t = block(10000, 1000, 203, 1, w_nan);
        EXPECT(tone_map_check(&t) != nullptr, "a NaN weight");
        t = block(10000, 1000, 203, 1, w_inf);
        EXPECT(tone_map_check(&t) != nullptr, "an infinite weight");
        t = block(10000, 1000, 203, 1, w_zero);
        EXPECT(tone_map_check(&t) != nullptr, "a zero weight sum");
        t = block(10000, 1000, 203, 1, w_neg);
        EXPECT(tone_map_check(&t) != nullptr, "a negative weight sum");
        t = block(10000, 1000, 203, 1, w_big);
        EXPECT(tone_map_check(&t) != nullptr, "a weight sum above 2");
        t = block(10000, 1000, 203, 1, w_two);
        EXPECT(tone_map_check(&t) == nullptr, "a weight sum of exactly 2");
    }
    // ---- the constants ----
    for (const auto& t : good) {
        ToneMapArgs a;
        tone_map_fill(&t, &a);
        EXPECT(std::isfinite(a.e_src) && a.e_src > 0.0f && a.e_src <= 1.0f, "e_src in (0, 1]");
        EXPECT(std::isfinite(a.max_lum) && a.max_lum > 0.0f, "max_lum finite and positive");
        EXPECT(a.ks == (float)(1.5 * (tm_pq_inv((double)t.target_nits) / tm_pq_inv((double)t.source_nits)) - 0.5), "ks rounded once");
        EXPECT(a.norm == (float)((double)t.unit_nits / (double)t.target_nits), "norm rounded once");
        EXPECT((t.source_nits <= t.target_nits) == (a.max_lum >= 1.0f), "max_lum >= 1 exactly when there is nothing to compress");
    }
    EXPECT(std::fabs(tm_pq_inv(10000.0) - 1.0) < 1e-15 && tm_pq_inv(0.0) < 1e-6, "pq_inv at the ends");
    for (double L : {0.01, 1.0, 100.0, 203.0, 1000.0, 9999.0}) EXPECT(std::fabs(tm_pq(tm_pq_inv(L)) / L - 1.0) < 1e-12, "pq(pq_inv(L)) == L");
    // ---- the operator ----
    for (const auto& t : good) {
        ToneMapArgs a;
        tone_map_fill(&t, &a);
        const float peak = t.source_nits / t.unit_nits;
        float g[3] = {peak, peak, peak};
        tone_map_pixel(a, g);
        const float want = t.source_nits <= t.target_nits ? peak * a.norm : 1.0f;  // nothing to compress: the identity times norm
        for (float v : g) EXPECT(std::fabs(v - want) <= 4e-6f * want, "a grey pixel at the content's peak comes out at the display's");
        float prev = 0.0f;
        for (int i = 0; i <= 2000; i++) {  // a grey ramp is non-decreasing (up to the float rounding of one product)
            const float x = peak * 1.25f * (float)i / 2000.0f;
            float v[3] = {x, x, x};
            tone_map_pixel(a, v);
            EXPECT(std::isfinite(v[0]) && v[0] >= prev * (1.0f - 1e-6f), "a grey ramp is non-decreasing");
            prev = v[0];
        }
        for (int i = 0; i < 4000; i++) {
            const float scale = t.source_nits / t.unit_nits * 1.5f;
            float v[3] = {(rnd() * 1.3f - 0.15f) * scale, (rnd() * 1.3f - 0.15f) * scale, (rnd() * 1.3f - 0.15f) * scale};
            if (i % 97 == 0) v[i % 3] = 0.0f;
            const float in[3] = {v[0], v[1], v[2]};
            tone_map_pixel(a, v);
            for (int c = 0; c < 3; c++) {
                EXPECT(std::isfinite(v[c]), "finite in, finite out");
                if (t.gamut) EXPECT(v[c] >= -1e-6f && v[c] <= 1.0f + 1e-6f, "with the gamut step every sample is in [0, 1]");
            }
            if (!t.gamut) {  // one factor for the three samples
                const float Y = (a.lum[0] * in[0] + a.lum[1] * in[1]) + a.lum[2] * in[2];
                const float r = tone_map_ratio(a, Y);
                for (int c = 0; c < 3; c++) EXPECT(v[c] == in[c] * r, "the channel ratios are kept");
            }
        }
        float n[3] = {nan, 0.25f, 0.5f};
        tone_map_pixel(a, n);
        EXPECT(n[0] != n[0], "NaN maps to NaN");
    }
    for (int i = 1; i + 6 < argc; i += 7) {
        const jxl_tone_map t = block((float)atof(argv[i]), (float)atof(argv[i + 1]), (float)atof(argv[i + 2]), atoi(argv[i + 3]));
        const char* why = tone_map_check(&t);
        if (why) {
            printf("REFUSED %s\n", why);
            continue;
        }
        ToneMapArgs a;
        tone_map_fill(&t, &a);
        float v[3] = {(float)atof(argv[i + 4]), (float)atof(argv[i + 5]), (float)atof(argv[i + 6])};
        tone_map_pixel(a, v);
        printf("PIXEL %.9g %.9g %.9g\n", v[0], v[1], v[2]);
    }
    printf("%d failure(s)\n", failures);
    return failures ? 1 : 0;
}
