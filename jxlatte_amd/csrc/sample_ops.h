// The reference's per-sample arithmetic, defined once: Java's (int)float, ImageBuffer.castToInt0, OpsinInverseMatrix.invertXYB of
// one pixel, the PQ / sRGB fromLinearF curves and the rule that picks a threshold-table quantiser. Every kernel that restates one
// of these stages (k_restore.hip, the sinks of restore_sink.h, the colour kernels of color_samples.h, k_post.hip) and the host code
// that needs the cast (spline_host.hip) calls these functions, so they evaluate the very same float operations by construction.
// Include from a file compiled with -ffp-contract=off.
#pragma once
#include "jxl_fastpow.h"
#include "jxl_internal.h"

namespace jxl {

// Java (int)float: NaN -> 0, saturating
__host__ __device__ __forceinline__ int32_t java_f2i(float v) {
    if (v != v) return 0;
    if (v >= 2147483648.0f) return INT32_MAX;
    if (v <= -2147483648.0f) return INT32_MIN;
    return (int32_t)v;
}

// ImageBuffer.castToInt0 (ImageBuffer.java:129-147)
__host__ __device__ __forceinline__ int32_t cast_to_int0(float v, int max_value) {
    const int32_t q = java_f2i(v * (float)max_value + 0.5f);
    return q < 0 ? 0 : q > max_value ? max_value : q;
}

// ImageBuffer.castToFloat0 (ImageBuffer.java:112-127) of one sample, scale = 1f / max: the conversion rounded first, then one
// f32 multiply (k_modular_to_float's expression; no contraction can join the two)
__host__ __device__ __forceinline__ float cast_to_float0(int32_t v, float scale) { return scale * (float)v; }

// OpsinInverseMatrix.invertXYB of one pixel (OpsinInverseMatrix.java:124-139)
__device__ __forceinline__ void invert_xyb_px(const XybParams& p, float& X, float& Y, float& B) {
    const float gammaL = Y + X + p.cob[0];
    const float gammaM = Y - X + p.cob[1];
    const float gammaS = B + p.cob[2];
    const float mixL = (gammaL * gammaL) * gammaL + p.ob[0];
    const float mixM = (gammaM * gammaM) * gammaM + p.ob[1];
    const float mixS = (gammaS * gammaS) * gammaS + p.ob[2];
    X = p.sm[0] * mixL + p.sm[1] * mixM + p.sm[2] * mixS;
    Y = p.sm[3] * mixL + p.sm[4] * mixM + p.sm[5] * mixS;
    B = p.sm[6] * mixL + p.sm[7] * mixM + p.sm[8] * mixS;
}

// TF_PQ.fromLinear through the default fromLinearF (TransferFunction.java:83-87, 104-106: double pow, result cast to float) and
// TF_SRGB.fromLinearF (:39-44), through jxl_fastpow.h (~110 instead of 463 instructions for the PQ curve, float results identical
// on all sampled inputs). The JXL_EXACT_POW experiment build has ocml's pow() instead and no table forms, for comparison -- in
// EVERY kernel that goes through this header: the colour kernels, which used to keep jxl_fastpow.h's forms in that build, follow
// it too. The default build is what it was.
#ifdef JXL_EXACT_POW
constexpr bool kExactPow = true;
__device__ __forceinline__ float tf_pq(float f) {
    const double d = pow((double)f, 0.159423828125);
    return (float)pow((0.8359375 + 18.8515625 * d) / (1.0 + 18.6875 * d), 78.84375);
}
__device__ __forceinline__ float tf_srgb(float f) {
    if (f < 0.00313066844250063f) return f * 12.92f;
    return 1.055f * (float)pow((double)f, 0.4166666666666667) + -0.055f;
}
#else
constexpr bool kExactPow = false;
__device__ __forceinline__ float tf_pq(float f) { return fp_tf_pq(f); }
__device__ __forceinline__ float tf_srgb(float f) { return fp_tf_srgb(f); }
#endif

// TransferFunction.fromLinearF of JXL_TRANSFER_PQ / JXL_TRANSFER_SRGB as a float (anything else: v as it is); PQ through the
// segment table (kPqTableFloats floats) when there is one
__device__ __forceinline__ float from_linear_f(float v, int transfer, const float* pq_tab) {
    if (!kExactPow && transfer == JXL_TRANSFER_PQ && pq_tab) v = fp_tf_pq_tab(v, reinterpret_cast<const float4*>(pq_tab));
    else if (transfer == JXL_TRANSFER_PQ) v = tf_pq(v);
    else if (transfer == JXL_TRANSFER_SRGB) v = tf_srgb(v);
    return v;
}

// fromLinearF + castToInt0 of one sample (max_value > 0): the threshold-table forms of jxl_fastpow.h where (transfer, max_value)
// has one and its tables are there (the oracle's integer for every input), else the float curve and the Java cast
__device__ __forceinline__ int32_t transfer_quant(float t, int transfer, int max_value, const float* pq_tab, const float* srgb8_tab,
                                                  const float* pq16_thr, const float* srgb16_tab) {
    if (!kExactPow) {
        if (transfer == JXL_TRANSFER_PQ && max_value == 65535 && pq_tab && pq16_thr)
            return fp_pq16(t, reinterpret_cast<const float4*>(pq_tab), pq16_thr);
        if (transfer == JXL_TRANSFER_PQ && max_value == 255 && pq16_thr) return fp_pq8(t, pq16_thr + kPq8ThrOffset);
        if (transfer == JXL_TRANSFER_SRGB && max_value == 65535 && srgb16_tab)
            return fp_srgb16(t, reinterpret_cast<const float4*>(srgb16_tab), srgb16_tab + kSrgb16ThrOffset);
        if (transfer == JXL_TRANSFER_SRGB && max_value == 255 && srgb8_tab) return fp_srgb8(t, reinterpret_cast<const float4*>(srgb8_tab));
    }
    return cast_to_int0(from_linear_f(t, transfer, pq_tab), max_value);
}

}  // namespace jxl
