// HDR -> SDR per pixel: the BT.2408 Annex 5 luminance curve on the pixel's own luminance, then the least desaturation that
// brings the pixel into [0, 1]. Not the reference's (ToneMapping.java only reads header fields, JXLImage.toneMapLinear is a
// primaries matrix): a capability beside it, defined by this comment. Plain C++ for host and device: the colour kernels call it
// behind their matrix stage (color_samples.h: color_front), tools/native/tone_map_check.cpp runs it on the host. Include from a
// file compiled with -ffp-contract=off: every product and sum below is rounded on its own.
//
// PQ is the standard's (SMPTE ST 2084), NOT to_linear(JXL_TF_PQ) of color_samples.h, which restates the reference and has
// "+ 18.6875 d" in its denominator where the standard has "-":
//     m1 = 0.1593017578125, m2 = 78.84375, c1 = 0.8359375, c2 = 18.8515625, c3 = 18.6875
//     pq_inv(L) = ((c1 + c2 p) / (1 + c3 p))^m2,  p = (L / 10000)^m1                           nits -> signal
//     pq(e)     = 10000 (max(q - c1, 0) / (c2 - c3 q))^(1 / m1),  q = e^(1 / m2)               signal -> nits
// both in double. The powers and quotients of the two functions are fp_pow / fp_div (jxl_fastpow.h) on the device and
// std::pow and "/" on the host; every other operation is the plain double one.
//
// The block (ToneMapArgs) is filled by the host (tone_map_check.h: tone_map_fill), each derived constant computed in double and
// rounded ONCE to float:
//     e_src = pq_inv(source_nits)   max_lum = pq_inv(target_nits) / e_src   ks = 1.5 max_lum - 0.5   norm = unit_nits / target_nits
// Below, a float of the block that enters a double expression is widened first.
//
// One pixel, v[3] linear samples in the TARGET primaries (a grey image filled to three equal samples first):
//   1. float   Y = (lum0 v0 + lum1 v1) + lum2 v2
//   2. ratio = norm when !(Y > 0) (zero, negative, NaN), or max_lum >= 1, or E1 < ks, where
//        double  Ln = (double)Y * unit_nits,  e = pq_inv(Ln),  E1 = e / e_src  (a plain double division)
//      No PQ round trip is taken for such a pixel: norm == 1.0f leaves its samples bit for bit.
//   3. otherwise, all in double:
//        E1 = min(E1, 1)    T = (E1 - ks) / (1 - ks)    T2 = T T    T3 = T2 T
//        E2 = (((2 T3 - 3 T2) + 1) ks + ((T3 - 2 T2) + T) (1 - ks)) + (3 T2 - 2 T3) max_lum       (Annex 5 with Lb = 0: no black lift)
//        E2 = E2 > 0 ? E2 : 0                (only a target so far below the source that ks < 0 gets here: the spline dips below 0)
//        Lp = pq(E2 * e_src)
//        float ratio = (float)(Lp / Ln) * norm                        (a plain double division, one rounding, a float product)
//   4. float   v[c] = v[c] * ratio                                    (hue and saturation kept)
//   5. when gamut, all in float, every comparison false on a NaN:
//        Yo = Y * ratio;  Yo = Yo < 0 ? 0 : Yo > 1 ? 1 : Yo           (a NaN stays)
//        t_c = v_c < 0 ? v_c / (v_c - Yo) : v_c > 1 ? (v_c - 1) / (v_c - Yo) : 0
//        t = 0; for c = 0, 1, 2: if (t_c > t) t = t_c;   if (t > 1) t = 1
//        if (t > 0) v_c = v_c + t * (Yo - v_c)                        (a pixel inside [0, 1] is left bit for bit)
// The scale stage (stage 5 of color_samples.h) is not applied to a tone-mapped pixel.
#ifndef JXL_TONE_MAP_OPS_H
#define JXL_TONE_MAP_OPS_H

#if defined(__HIPCC__)
#include "jxl_fastpow.h"
#define JXL_TM_FN __host__ __device__ inline
#else
#define JXL_TM_FN inline
#endif
#if !defined(__HIP_DEVICE_COMPILE__)
#include <cmath>
#endif

namespace jxl {

struct ToneMapArgs {
    float lum[3];                             // the Y row of the target primaries' RGB -> XYZ matrix
    float unit_nits, source_nits, target_nits;
    int gamut;                                // 0 or 1
    float e_src, max_lum, ks, norm;           // tone_map_fill
};

JXL_TM_FN double tm_pow(double x, double p) {
#if defined(__HIP_DEVICE_COMPILE__)
    return fp_pow(x, p);
#else
    return std::pow(x, p);
#endif
}

JXL_TM_FN double tm_div(double a, double b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return fp_div(a, b);
#else
    return a / b;
#endif
}

// nits -> PQ signal; L >= 0
JXL_TM_FN double tm_pq_inv(double L) {
    const double p = tm_pow(L / 10000.0, 0.1593017578125);
    return tm_pow(tm_div(0.8359375 + 18.8515625 * p, 1.0 + 18.6875 * p), 78.84375);
}

// PQ signal -> nits; e >= 0
JXL_TM_FN double tm_pq(double e) {
    const double q = tm_pow(e, 1.0 / 78.84375);
    double num = q - 0.8359375;
    if (!(num > 0.0)) num = 0.0;
    return 10000.0 * tm_pow(tm_div(num, 18.8515625 - 18.6875 * q), 1.0 / 0.1593017578125);
}

// steps 2 and 3: the factor of a pixel of luminance Y
JXL_TM_FN float tone_map_ratio(const ToneMapArgs& a, float Y) {
    if (!(Y > 0.0f) || a.max_lum >= 1.0f) return a.norm;
    const double ks = (double)a.ks;
    const double Ln = (double)Y * (double)a.unit_nits;
    double E1 = tm_pq_inv(Ln) / (double)a.e_src;
    if (E1 < ks) return a.norm;
    if (E1 > 1.0) E1 = 1.0;
    const double T = (E1 - ks) / (1.0 - ks);
    const double T2 = T * T, T3 = T2 * T;
    double E2 = (((2.0 * T3 - 3.0 * T2) + 1.0) * ks + ((T3 - 2.0 * T2) + T) * (1.0 - ks)) + (3.0 * T2 - 2.0 * T3) * (double)a.max_lum;
    if (!(E2 > 0.0)) E2 = 0.0;
    const double Lp = tm_pq(E2 * (double)a.e_src);
    return (float)(Lp / Ln) * a.norm;
}

// steps 1 - 5 on the three samples of one pixel, in place
JXL_TM_FN void tone_map_pixel(const ToneMapArgs& a, float v[3]) {
    const float Y = (a.lum[0] * v[0] + a.lum[1] * v[1]) + a.lum[2] * v[2];
    const float ratio = tone_map_ratio(a, Y);
    for (int c = 0; c < 3; c++) v[c] = v[c] * ratio;
    if (!a.gamut) return;
    float Yo = Y * ratio;
    Yo = Yo < 0.0f ? 0.0f : Yo > 1.0f ? 1.0f : Yo;
    float t = 0.0f;
    for (int c = 0; c < 3; c++) {
        const float tc = v[c] < 0.0f ? v[c] / (v[c] - Yo) : v[c] > 1.0f ? (v[c] - 1.0f) / (v[c] - Yo) : 0.0f;
        if (tc > t) t = tc;
    }
    if (t > 1.0f) t = 1.0f;
    if (t > 0.0f)
        for (int c = 0; c < 3; c++) v[c] = v[c] + t * (Yo - v[c]);
}

}  // namespace jxl
#endif  // JXL_TONE_MAP_OPS_H
