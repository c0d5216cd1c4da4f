// One cell of the LF stage, defined once: LF dequantisation + LF chroma-from-luma (LFCoefficients.java:66-95) and adaptiveSmooth
// (:113-180) of the cell at (y, x) of ONE LF group. k_lf.hip (the LF planes the IDCT stage reads) and k_lf_image.hip (the LF image
// as the picture at 1:8) both call it, so they evaluate the very same float operations. Include from a file compiled with
// -ffp-contract=off.
//
// A: anything with q[3] (lfQuant in X, Y, B order, [H][W] of the LF group), H, W, sd[3] (scaledDequant[i] / (1 << extraPrecision)),
// sd_gap[3] (scaledDequant[i]), kX, kB and smooth.
#pragma once
#include "jxl_internal.h"

namespace jxl {

// dequantised + CfL'd LF sample of the three channels at (y, x) (LFCoefficients.java:66-95)
template <typename A>
__device__ __forceinline__ void lf_sample(const A& a, int y, int x, float v[3]) {
    const int k = y * a.W + x;
    const float yv = (float)a.q[1][k] * a.sd[1];
    v[1] = yv;
    v[0] = (float)a.q[0][k] * a.sd[0] + a.kX * yv;
    v[2] = (float)a.q[2][k] * a.sd[2] + a.kB * yv;
}

// the cell's three output samples; 0 <= y < a.H, 0 <= x < a.W. The 3x3 neighbourhood is re-dequantised from the integer LF image
// (9 x 3 int loads, L1/L2 hits) instead of staging a float image
template <typename A>
__device__ __forceinline__ void lf_cell(const A& a, int y, int x, float o[3]) {
    float c[3];
    lf_sample(a, y, x, c);
    o[0] = c[0];
    o[1] = c[1];
    o[2] = c[2];
    if (a.smooth && y > 0 && y + 1 < a.H && x > 0 && x + 1 < a.W) {  // adaptiveSmooth (:113-180); border cells are copied
        float nb[3][3][3];  // [dy][dx][channel]
#pragma unroll
        for (int dy = 0; dy < 3; dy++)
#pragma unroll
            for (int dx = 0; dx < 3; dx++) lf_sample(a, y + dy - 1, x + dx - 1, nb[dy][dx]);
        float gap = 0.5f;
        float w[3];
#pragma unroll
        for (int i = 0; i < 3; i++) {
            const float sample = nb[1][1][i];
            const float adjacent = nb[1][0][i] + nb[1][2][i] + nb[0][1][i] + nb[2][1][i];
            const float diag = nb[0][0][i] + nb[0][2][i] + nb[2][0][i] + nb[2][2][i];
            w[i] = 0.05226273532324128f * sample + 0.20345139757231578f * adjacent + 0.0334829185968739f * diag;
            const float g = fabsf(sample - w[i]) * a.sd_gap[i];
            if (g > gap) gap = g;
        }
        const float t = 3.0f - 4.0f * gap;
        gap = t > 0.0f ? t : 0.0f;  // Math.max(0f, 3f - 4f * g)
#pragma unroll
        for (int i = 0; i < 3; i++) o[i] = (c[i] - w[i]) * gap + w[i];
    }
}

}  // namespace jxl
