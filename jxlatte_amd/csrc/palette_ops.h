// The inverse Palette transform's per-sample arithmetic, defined once: the colour an index names (ModularStream.java:341-366)
// and ModularChannel.prediction for the predictors a palette can name (ModularChannel.java:143-183, with the edge fallbacks of
// :95-121). The kernels of k_palette.hip and the host loop of tools/native/palette_check.cpp call these functions, so they
// evaluate the very same integer operations by construction. __host__ __device__ under hipcc, plain C++ under any other
// compiler (no device code, no context).
//
// Everything follows Java `int` semantics: every sum, product, negation and left shift wraps at 32 bits (done in uint32_t
// here: signed overflow and a left shift of a negative value are not defined in C++), `/` and `%` truncate toward zero (as
// C++'s do), and a shift count is taken mod 32 (index >> (2 * c) for c >= 16, 1 << bit_depth for bit_depth = 32).
#pragma once
#include <stdint.h>

#include "../../include/jxl_tables.h"

#if defined(__HIPCC__)
#define JXL_PAL_FN __host__ __device__ __forceinline__
#define JXL_PAL_TABLE __device__ __constant__
#else
#define JXL_PAL_FN inline
#endif

namespace jxl {

// Java's int operators
JXL_PAL_FN int32_t jadd(int32_t a, int32_t b) { return (int32_t)((uint32_t)a + (uint32_t)b); }
JXL_PAL_FN int32_t jsub(int32_t a, int32_t b) { return (int32_t)((uint32_t)a - (uint32_t)b); }
JXL_PAL_FN int32_t jmul(int32_t a, int32_t b) { return (int32_t)((uint32_t)a * (uint32_t)b); }
JXL_PAL_FN int32_t jneg(int32_t a) { return (int32_t)(0u - (uint32_t)a); }
JXL_PAL_FN int32_t jshl(int32_t a, int32_t n) { return (int32_t)((uint32_t)a << (n & 31)); }
JXL_PAL_FN int32_t jshr(int32_t a, int32_t n) { return a >> (n & 31); }  // arithmetic, as Java's >>
JXL_PAL_FN int32_t jabs(int32_t a) { return a < 0 ? jneg(a) : a; }      // Math.abs: INT32_MIN stays INT32_MIN

// kDeltaPalette (ModularStream.java:20-33); device code reads a copy of its own in constant memory
#if defined(__HIPCC__)
static JXL_PAL_TABLE const int16_t kDeltaPaletteDev[JXL_DELTA_PALETTE_ROWS][3] = JXL_DELTA_PALETTE_INIT;
#endif
static const int16_t kDeltaPaletteHost[JXL_DELTA_PALETTE_ROWS][3] = JXL_DELTA_PALETTE_INIT;

JXL_PAL_FN int32_t delta_palette(int32_t row, int32_t c) {
#if defined(__HIP_DEVICE_COMPILE__)
    return kDeltaPaletteDev[row][c];
#else
    return kDeltaPaletteHost[row][c];
#endif
}

// what palette_value needs of a jxl_palette_desc; `palette` holds row c at palette + c * pal_w (the caller may have copied the
// rows elsewhere, with another stride)
struct PaletteLookup {
    const int32_t* palette;
    int32_t pal_w, nb_colors, bit_depth;
};

// ModularStream.java:344-366: the value of `index` in channel c. Reads palette[c * pal_w + index] only for 0 <= index <
// nb_colors (palette_check.h has made that read safe); c >= 0.
JXL_PAL_FN int32_t palette_value(int32_t index, int32_t c, const PaletteLookup& d) {
    if (index >= 0 && index < d.nb_colors) return d.palette[(int64_t)c * d.pal_w + index];
    const int32_t max_value = jsub(jshl(1, d.bit_depth), 1);  // (1 << bitDepth) - 1: 0 for 32, INT32_MAX for 31
    if (index >= d.nb_colors) {
        index -= d.nb_colors;  // both >= 0 here: no wrap
        if (index < 64) {
            const int32_t step = jshr(index, 2 * c) % 4;
            const int32_t shift = d.bit_depth - 3 > 0 ? d.bit_depth - 3 : 0;
            return jadd(jmul(step, max_value) / 4, jshl(1, shift));
        }
        index -= 64;
        for (int32_t k = 0; k < c && index != 0; k++) index /= 5;  // (0 stays 0: the loop may stop there)
        return jmul(index % 5, max_value) / 4;
    }
    if (c >= 3) return 0;
    index = jsub(jneg(index), 1) % 143;  // -index - 1 of a negative int: 0 .. INT32_MAX, INT32_MIN included
    int32_t value = delta_palette((index + 1) >> 1, c);
    if ((index & 1) == 0) value = -value;
    if (d.bit_depth > 8) value = jshl(value, (d.bit_depth < 24 ? d.bit_depth : 24) - 8);
    return value;
}

// ModularChannel.prediction (ModularChannel.java:143-183) of predictors 0-5 and 7-13 from the seven neighbours, the edge
// fallbacks (:95-121) already applied (palette_neighbours). Predictor 6 reads the weighted predictor's plane instead and is the
// caller's ((pred + 3) >> 3, :165); it and every other k give 0 here.
JXL_PAL_FN int32_t palette_predict(int32_t k, int32_t W, int32_t N, int32_t NW, int32_t NE, int32_t NN, int32_t WW, int32_t NEE) {
    switch (k) {
        case 1: return W;
        case 2: return N;
        case 3: return jadd(W, N) / 2;
        case 4: return jabs(jsub(N, NW)) < jabs(jsub(W, NW)) ? W : N;
        case 5: {
            const int32_t v = jsub(jadd(W, N), NW);
            const int32_t lower = N < W ? N : W, upper = lower ^ N ^ W;  // MathHelper.clamp(v, n, w) (MathHelper.java:209-213)
            return v < lower ? lower : v > upper ? upper : v;
        }
        case 7: return NE;
        case 8: return NW;
        case 9: return WW;
        case 10: return jadd(W, NW) / 2;
        case 11: return jadd(N, NW) / 2;
        case 12: return jadd(N, NE) / 2;
        case 13: {
            int32_t s = jsub(jmul(6, N), jmul(2, NN));
            s = jadd(s, jmul(7, W));
            s = jadd(s, WW);
            s = jadd(s, NEE);
            s = jadd(s, jmul(3, NE));
            return jadd(s, 8) / 16;
        }
        default: return 0;
    }
}

// The seven neighbours of (x, y) in a plane of rows `w` wide, with the fallbacks of ModularChannel.java:95-121; every sample
// read lies before (x, y) in raster order, the farthest to the right being (x + 2, y - 1). nb = {W, N, NW, NE, NN, WW, NEE}.
JXL_PAL_FN void palette_neighbours(const int32_t* p, int32_t w, int32_t x, int32_t y, int32_t nb[7]) {
    const int32_t* row = p + (int64_t)y * w;
    const int32_t* up = y > 0 ? row - w : row;  // read only where y > 0
    const int32_t W = x > 0 ? row[x - 1] : y > 0 ? up[x] : 0;
    const int32_t N = y > 0 ? up[x] : x > 0 ? row[x - 1] : 0;
    const int32_t NW = x > 0 ? (y > 0 ? up[x - 1] : row[x - 1]) : (y > 0 ? up[x] : 0);
    const int32_t NE = x + 1 < w && y > 0 ? up[x + 1] : N;
    nb[0] = W;
    nb[1] = N;
    nb[2] = NW;
    nb[3] = NE;
    nb[4] = y > 1 ? row[x - 2 * (int64_t)w] : N;
    nb[5] = x > 1 ? row[x - 2] : W;
    nb[6] = x + 2 < w && y > 0 ? up[x + 2] : NE;
}

JXL_PAL_FN int32_t palette_predict_at(int32_t k, const int32_t* p, int32_t w, int32_t x, int32_t y) {
    int32_t nb[7];
    palette_neighbours(p, w, x, y, nb);
    return palette_predict(k, nb[0], nb[1], nb[2], nb[3], nb[4], nb[5], nb[6]);
}

// predictor 6 (:165) from the weighted predictor's value as decoded
JXL_PAL_FN int32_t palette_predict_wp(int32_t pred) { return jadd(pred, 3) >> 3; }

// a delta pixel's prediction does not depend on its neighbours for these predictors: the lookup kernel finishes it
JXL_PAL_FN bool palette_pred_is_local(int32_t d_pred) { return d_pred == 0 || d_pred == 6; }

}  // namespace jxl
