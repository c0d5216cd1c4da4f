// Colour management of JXLImage.transform (J/JXLImage.java:185-286) as one pass over the colour planes, and the reduction of
// JXLImage.determinePeak (:214-223) over the same front stages.
//
//   k_color_convert, per pixel, every stage switchable (ColorArgs):
//     1. cast        int32 -> float, v * (1.0f / max)                      ImageBuffer.castToFloat0 (ImageBuffer.java:112-127)
//     2. toLinearF   of the tagged transfer                                 TransferFunction.java:55-60, 73-78, 89-92, GammaTransferFunction
//     3. grey -> RGB three copies of the one plane (when a matrix follows)  JXLImage.fillColor (:141-164)
//     4. matrix      (m0 a + m1 b) + m2 c, every product and sum a float    MathHelper.matrixMutliply3InPlace
//     5. scale       f * scale (peak detection)                             JXLImage.java:278-280
//     6. fromLinearF of the target                                          TransferFunction.java:39-44, 65-70, 83-87, GammaTransferFunction
//     7. quantise    (int)(v * max + 0.5f), clamped                         ImageBuffer.castToInt0 (:129-145)
//   The scale follows the matrix: JXLImage.transform runs toneMapLinear BEFORE transfer(), and transfer() is where the peak is
//   taken (of the tone-mapped image) and applied.
//
// The reference treats the samples independently (the matrix mixes the three of one pixel): a grid-stride map, no LDS. The cost
// is double-precision VALU: ~110 f64 operations per fp_pow (jxl_fastpow.h). Every stage selector is a kernel argument, so the
// branches on them are scalar; what diverges inside a wave is only the reference's own per-sample branching (the linear
// segment of sRGB / BT.709; zero, negative, infinite and NaN bases of a pow), and there the wave runs the f64 chain at most
// once per pow, for the lanes that need it (skipped when none does).
// The three channels go through the chains one after the other: one fp_pow is live at a time.
#include "jxl_fastpow.h"
#include "jxl_internal.h"

namespace jxl {
namespace {

// Java (int)float: NaN -> 0, saturating
__device__ __forceinline__ int32_t f2i(float v) {
    if (v != v) return 0;
    if (v >= 2147483648.0f) return INT32_MAX;
    if (v <= -2147483648.0f) return INT32_MIN;
    return (int32_t)v;
}

// ImageBuffer.castToInt0 (ImageBuffer.java:129-145)
__device__ __forceinline__ int32_t to_int(float v, int max_value) {
    const int32_t q = f2i(v * (float)max_value + 0.5f);
    return q < 0 ? 0 : q > max_value ? max_value : q;
}

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

// TransferFunction.fromLinearF as a float. LINEAR / SRGB / PQ: the functions jxl_stage_transfer evaluates (k_restore.hip,
// apply_transfer: PQ through the segment table when the context has one).
__device__ __forceinline__ float from_linear(float v, int tf, double p, int kind, const float4* pq_tab) {
    if (tf == JXL_TF_SRGB) return fp_tf_srgb(v);
    if (tf == JXL_TF_PQ) return pq_tab ? fp_tf_pq_tab(v, pq_tab) : fp_tf_pq(v);
    if (tf == JXL_TF_BT709) {  // :65-70
        const double d = (double)v;
        if (d < 0.018053968510807807336) return (float)(4.5 * d);
        return (float)(1.0992968268094429403 * fp_pow(d, 0.45) - 0.0992968268094429403);
    }
    if (tf == JXL_TF_GAMMA) return (float)pow_any((double)v, p, kind);  // GammaTransferFunction.fromLinear
    return v;
}

// stages 6 + 7 with integer output: the exact threshold tables of k_transfer where it uses them, else float + castToInt0
__device__ __forceinline__ int32_t from_linear_int(float v, const ColorArgs& a) {
    if (a.tf_out == JXL_TF_PQ && a.max_value == 65535 && a.pq_tab && a.pq16_thr)
        return fp_pq16(v, reinterpret_cast<const float4*>(a.pq_tab), a.pq16_thr);
    if (a.tf_out == JXL_TF_PQ && a.max_value == 255 && a.pq16_thr) return fp_pq8(v, a.pq16_thr + 65537);
    if (a.tf_out == JXL_TF_SRGB && a.max_value == 65535 && a.srgb16_tab)
        return fp_srgb16(v, reinterpret_cast<const float4*>(a.srgb16_tab), a.srgb16_tab + kSrgb8TableFloats);
    if (a.tf_out == JXL_TF_SRGB && a.max_value == 255 && a.srgb8_tab) return fp_srgb8(v, reinterpret_cast<const float4*>(a.srgb8_tab));
    return to_int(from_linear(v, a.tf_out, a.p_out, a.kind_out, reinterpret_cast<const float4*>(a.pq_tab)), a.max_value);
}

// stages 1 + 2 of sample i of input plane c
__device__ __forceinline__ float linear_sample(const ColorArgs& a, int c, int64_t i) {
    const float f = a.in_is_int ? (float)((const int32_t*)a.in[c])[i] * a.in_scale[c] : ((const float*)a.in[c])[i];
    return to_linear(f, a.tf_in, a.p_in, a.kind_in);
}

__device__ __forceinline__ void store_sample(const ColorArgs& a, int c, int64_t i, float v) {
    if (a.max_value > 0) ((int32_t*)a.out[c])[i] = from_linear_int(v, a);
    else ((float*)a.out[c])[i] = from_linear(v, a.tf_out, a.p_out, a.kind_out, reinterpret_cast<const float4*>(a.pq_tab));
}

}  // namespace

__global__ __launch_bounds__(256) void k_color_convert(const ColorArgs a) {
    for (int64_t i = blockIdx.x * 256LL + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * 256) {
        float r = linear_sample(a, 0, i);
        if (a.n_planes == 1 && !a.use_matrix) {  // grey stays grey
            if (a.use_scale) r = r * a.scale;
            store_sample(a, 0, i, r);
            continue;
        }
        float g = r, b = r;  // fillColor
        if (a.n_planes == 3) {
            g = linear_sample(a, 1, i);
            b = linear_sample(a, 2, i);
        }
        if (a.use_matrix) {
            const float x = (a.m[0] * r + a.m[1] * g) + a.m[2] * b;
            const float y = (a.m[3] * r + a.m[4] * g) + a.m[5] * b;
            const float z = (a.m[6] * r + a.m[7] * g) + a.m[8] * b;
            r = x; g = y; b = z;
        }
        if (a.use_scale) {
            r = r * a.scale; g = g * a.scale; b = b * a.scale;
        }
        store_sample(a, 0, i, r);
        store_sample(a, 1, i, g);
        store_sample(a, 2, i, b);
    }
}

void launch_color_convert(const ColorArgs& a, hipStream_t s) {
    if (a.n <= 0) return;
    int64_t grid = (a.n + 255) / 256;
    if (grid > 8192) grid = 8192;
    hipLaunchKernelGGL(k_color_convert, dim3((unsigned)grid), dim3(256), 0, s, a);
}

// ---- JXLImage.determinePeak (:214-223) ---------------------------------------------------------------------------------------------
// Float planes: per row MathHelper.max(float...) (MathHelper.java:190-195), which starts from a[0] and keeps
// r = a[i] < r ? a[i] : r -- the row MINIMUM, with a NaN first sample sticking and later NaNs skipped, and of two zeros of
// different sign the one that comes first; then the maximum over rows in Float.compareTo order (NaN greatest, -0 < +0).
// The row rule is not associative as it stands; it is the same as
//     a[0] is NaN ? a[0] : the first sample, in row order, among those of least value, NaNs at i >= 1 read as +inf
// and THAT is a minimum over the key (value with +-0 equal, column, sign of a zero), which is associative: one 64-bit
// unsigned minimum per row, reduced in any order. Column 0 is kept apart for the NaN test.
// The row results go through an order-preserving map of compareTo to uint32 and one atomic maximum per row: the outcome does
// not depend on the order of arrival.
// The sample is that of determinePeak's plane after stages 1-4: green (plane 1) of three planes, plane 0 of a grey image, or the
// second row of the matrix when toneMapLinear ran first.
// An int32 plane that is linear already and has no matrix: the plain maximum (:219); the division is done by the host.
namespace {

__device__ __forceinline__ uint64_t row_key(float f, uint32_t x) {
    uint32_t b = __builtin_bit_cast(uint32_t, f);
    if (f != f) b = 0x7F800000u;  // a NaN beyond column 0 never wins: a[i] < r is false
    uint32_t zsign = 0;
    if ((b << 1) == 0u) {
        zsign = b >> 31;
        b = 0;
    }
    const uint32_t ord = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    return ((uint64_t)ord << 31) | ((uint64_t)x << 1) | zsign;  // x < 2^30
}

__device__ __forceinline__ float row_key_value(uint64_t key) {
    const uint32_t ord = (uint32_t)(key >> 31);
    uint32_t b = (ord & 0x80000000u) ? (ord & 0x7FFFFFFFu) : ~ord;
    if (b == 0u && (key & 1u)) b = 0x80000000u;
    return __builtin_bit_cast(float, b);
}

// Float.compareTo order as unsigned: NaN on top, -0 below +0
__device__ __forceinline__ uint32_t compare_key(float f) {
    if (f != f) return 0xFFFFFFFFu;
    const uint32_t b = __builtin_bit_cast(uint32_t, f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

}  // namespace

__global__ __launch_bounds__(256) void k_color_peak(const ColorArgs a, int h, int w, uint32_t* result) {
    __shared__ uint64_t red[256];
    const int tid = threadIdx.x;
    const int pc = a.n_planes == 3 ? 1 : 0;
    const bool int_max = a.in_is_int && a.tf_in == JXL_TF_LINEAR && !a.use_matrix;
    for (int row = blockIdx.x; row < h; row += gridDim.x) {
        const int64_t base = (int64_t)row * w;
        uint64_t key = ~0ull;
        uint32_t mx = 0;  // integer samples, biased to unsigned
        float first = 0.0f;
        for (int x = tid; x < w; x += 256) {
            if (int_max) {
                const uint32_t v = (uint32_t)((const int32_t*)a.in[pc])[base + x] ^ 0x80000000u;
                mx = v > mx ? v : mx;
                continue;
            }
            float f;
            if (a.use_matrix) {
                const float r = linear_sample(a, 0, base + x);
                const float g = a.n_planes == 3 ? linear_sample(a, 1, base + x) : r;
                const float b = a.n_planes == 3 ? linear_sample(a, 2, base + x) : r;
                f = (a.m[3] * r + a.m[4] * g) + a.m[5] * b;
            } else {
                f = linear_sample(a, pc, base + x);
            }
            if (x == 0) first = f;  // thread 0 only
            const uint64_t k = row_key(f, (uint32_t)x);
            key = k < key ? k : key;
        }
        red[tid] = int_max ? ~(uint64_t)mx : key;  // the integer maximum as the minimum of the complement: one reduction for both
        __syncthreads();
        for (int step = 128; step >= 1; step >>= 1) {
            if (tid < step) {
                const uint64_t o = red[tid + step];
                if (o < red[tid]) red[tid] = o;
            }
            __syncthreads();
        }
        if (tid == 0) {
            uint32_t k32;
            if (int_max) {
                k32 = (uint32_t)~red[0];
            } else {
                const float v = first != first ? first : row_key_value(red[0]);
                k32 = compare_key(v);
            }
            atomicMax(result, k32);
        }
        __syncthreads();
    }
}

void launch_color_peak(const ColorArgs& a, int h, int w, uint32_t* result, hipStream_t s) {
    if (h <= 0 || w <= 0) return;
    hipLaunchKernelGGL(k_color_peak, dim3((unsigned)(h < 4096 ? h : 4096)), dim3(256), 0, s, a, h, w, result);
}

}  // namespace jxl
