// The sample functions of the colour kernels (k_color.hip: k_color_convert, k_color_peak; k_png.hip: k_png_samples): the
// reference's casts, transfer curves and quantiser as device functions, so that every kernel that restates a stage of
// JXLImage.transform evaluates the very same float operations. Include from a file compiled with -ffp-contract=off.
#ifndef JXL_COLOR_SAMPLES_H
#define JXL_COLOR_SAMPLES_H
#include "sample_ops.h"

namespace jxl {
namespace {

// Math.pow(x, p) for any finite p > 0 (GammaTransferFunction: p = 1e7 / g or 1e-7 * g can be an integer, e.g. g = 5000000).
// kind: 0 p is not an integer, 1 an even integer, 2 an odd integer (host: pow_kind).
//   NaN -> NaN; +-0 -> +0 (-0 for -0 and odd p); +-inf -> +inf (-inf for -inf and odd p);
//   x < 0: NaN for a non-integer p, else +-|x|^p.
__device__ __forceinline__ double pow_any(double x, double p, int kind) {
    const double ax = __builtin_fabs(x);
    const bool neg = __builtin_signbit(x);
    const bool finite_pos = ax > 0.0 && ax < __builtin_inf();
    if (neg && kind == 0) return finite_pos || ax != ax ? __builtin_nan("") : ax;  // -0 -> +0, -inf -> +inf
    double r = ax;  // 0, inf, NaN
    if (finite_pos) r = fp_pow_pos(ax, p);
    return neg && kind == 2 ? -r : r;
}

// TransferFunction.toLinearF. sRGB has its own float form (:55-60); the others are the interface default
// (float)toLinear((double)f) (:100-102).
__device__ __forceinline__ float to_linear(float f, int tf, double p, int kind) {
    if (tf == JXL_TF_SRGB) {
        if (f < 0.0404482362771082f) return f * 0.07739938080495357f;
        return (float)fp_pow((double)(f * 0.9478672985781991f + 0.052132701f), 2.4);
    }
    if (tf == JXL_TF_BT709) {  // :73-78
        const double d = (double)f;
        if (d < 0.081242858298635133011) return (float)(d * 0.22222222222222222222);
        return (float)fp_pow((d + 0.0992968268094429403) * 0.90967241568627260377, 2.2222222222222222222);
    }
    if (tf == JXL_TF_PQ) {  // :89-92. f below ~7.3e-7 (zero included): d < 0.8359375, a negative base, NaN -- as in the reference
        const double d = fp_pow((double)f, 0.012683313515655965121);
        return (float)fp_pow(fp_div(d - 0.8359375, 18.8515625 + 18.6875 * d), 6.2725880551301684533);
    }
    if (tf == JXL_TF_GAMMA) return (float)pow_any((double)f, p, kind);  // GammaTransferFunction.toLinear
    return f;
}

// TransferFunction.fromLinearF as a float. LINEAR / SRGB / PQ: the functions jxl_stage_transfer evaluates (sample_ops.h,
// from_linear_f: PQ through the segment table when the context has one).
__device__ __forceinline__ float from_linear(float v, int tf, double p, int kind, const float* pq_tab) {
    if (tf == JXL_TF_SRGB) return from_linear_f(v, JXL_TRANSFER_SRGB, pq_tab);  // JXL_TF_* and JXL_TRANSFER_* number the curves differently
    if (tf == JXL_TF_PQ) return from_linear_f(v, JXL_TRANSFER_PQ, pq_tab);
    if (tf == JXL_TF_BT709) {  // :65-70
        const double d = (double)v;
        if (d < 0.018053968510807807336) return (float)(4.5 * d);
        return (float)(1.0992968268094429403 * fp_pow(d, 0.45) - 0.0992968268094429403);
    }
    if (tf == JXL_TF_GAMMA) return (float)pow_any((double)v, p, kind);  // GammaTransferFunction.fromLinear
    return v;
}

// stages 1 + 2 of one 4-byte sample word of input plane c
__device__ __forceinline__ float linear_word(const ColorArgs& a, int c, uint32_t word) {
    const float f = a.in_is_int ? (float)(int32_t)word * a.in_scale[c] : __builtin_bit_cast(float, word);
    return to_linear(f, a.tf_in, a.p_in, a.kind_in);
}

// tone_map_ops.h on one pixel. Inlined: out of line (__noinline__) every calling kernel got a stack -- 256 to 464 bytes of scratch
// per lane -- and lost more occupancy than the inlined branch's ~20 VGPRs cost (profiles/tone_map.md has both tables)
struct ToneMapped { float r, g, b; };
__device__ __forceinline__ ToneMapped tone_map_stage(const ToneMapArgs& tm, float r, float g, float b) {
    float v[3] = {r, g, b};
    tone_map_pixel(tm, v);
    return ToneMapped{v[0], v[1], v[2]};
}

// stages 1-5 of one pixel (cast, toLinearF, grey -> RGB, matrix, scale): the words of its colour planes (w[c], c < n_planes) ->
// COLORS linear float samples, COLORS being 3 when n_planes == 3, use_matrix or use_tone_map, else 1. With use_tone_map the tone
// mapping stands behind the matrix and the scale is not applied. What a kernel that filters in linear light
// (k_tensor_resize.hip) evaluates per SOURCE pixel; color_back is then its stage 6, per output sample
template <int COLORS>
__device__ __forceinline__ void color_front(const ColorArgs& a, const uint32_t w[3], float v[3]) {
    v[0] = linear_word(a, 0, w[0]);
    if (COLORS == 3) {
        v[1] = v[2] = v[0];  // fillColor
        if (a.n_planes == 3) {
            v[1] = linear_word(a, 1, w[1]);
            v[2] = linear_word(a, 2, w[2]);
        }
        if (a.use_matrix) {
            const float x = (a.m[0] * v[0] + a.m[1] * v[1]) + a.m[2] * v[2];
            const float y = (a.m[3] * v[0] + a.m[4] * v[1]) + a.m[5] * v[2];
            const float z = (a.m[6] * v[0] + a.m[7] * v[1]) + a.m[8] * v[2];
            v[0] = x; v[1] = y; v[2] = z;
        }
        if (a.use_tone_map) {
            const ToneMapped o = tone_map_stage(a.tm, v[0], v[1], v[2]);
            v[0] = o.r; v[1] = o.g; v[2] = o.b;
            return;
        }
    }
#pragma unroll
    for (int c = 0; c < COLORS; c++)
        if (a.use_scale) v[c] = v[c] * a.scale;
}

// stage 6 of one sample: fromLinearF of the output curve
__device__ __forceinline__ float color_back(const ColorArgs& a, float v) {
    return from_linear(v, a.tf_out, a.p_out, a.kind_out, a.pq_tab);
}

// stages 1-6 of one pixel as the writers' one-pass kernels (k_png.hip, k_tensor.hip) evaluate them
template <int COLORS>
__device__ __forceinline__ void color_stages(const ColorArgs& a, const uint32_t w[3], float v[3]) {
    color_front<COLORS>(a, w, v);
#pragma unroll
    for (int c = 0; c < COLORS; c++) v[c] = color_back(a, v[c]);
}

// stages 1 + 2 of sample i of input plane c
__device__ __forceinline__ float linear_sample(const ColorArgs& a, int c, int64_t i) {
    return linear_word(a, c, ((const uint32_t*)a.in[c])[i]);
}

}  // namespace
}  // namespace jxl
#endif  // JXL_COLOR_SAMPLES_H
