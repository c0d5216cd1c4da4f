// Colour management of JXLImage.transform (J/JXLImage.java:185-286) as one pass over the colour planes, and the reduction of
// JXLImage.determinePeak (:214-223) over the same front stages.
//
//   k_color_convert, per pixel, every stage switchable (ColorArgs):
//     1. cast        int32 -> float, v * (1.0f / max)                      ImageBuffer.castToFloat0 (ImageBuffer.java:112-127)
//     2. toLinearF   of the tagged transfer                                 TransferFunction.java:55-60, 73-78, 89-92, GammaTransferFunction
//     3. grey -> RGB three copies of the one plane (when a matrix follows)  JXLImage.fillColor (:141-164)
//     4. matrix      (m0 a + m1 b) + m2 c, every product and sum a float    MathHelper.matrixMutliply3InPlace
//     5. scale       f * scale (peak detection)                             JXLImage.java:278-280
//        or, with use_tone_map, the HDR -> SDR operator of tone_map_ops.h (not the reference's), which makes three planes of one
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
#include "color_samples.h"

namespace jxl {
namespace {

// stages 6 + 7 with integer output: sRGB and PQ as k_transfer quantises them (the exact threshold tables where it uses them),
// BT.709, gamma and linear as float + castToInt0
__device__ __forceinline__ int32_t from_linear_int(float v, const ColorArgs& a) {
    if (a.tf_out == JXL_TF_PQ) return transfer_quant(v, JXL_TRANSFER_PQ, a.max_value, a.pq_tab, a.srgb8_tab, a.pq16_thr, a.srgb16_tab);
    if (a.tf_out == JXL_TF_SRGB) return transfer_quant(v, JXL_TRANSFER_SRGB, a.max_value, a.pq_tab, a.srgb8_tab, a.pq16_thr, a.srgb16_tab);
    return cast_to_int0(from_linear(v, a.tf_out, a.p_out, a.kind_out, a.pq_tab), a.max_value);
}

__device__ __forceinline__ void store_sample(const ColorArgs& a, int c, int64_t i, float v) {
    if (a.max_value > 0) ((int32_t*)a.out[c])[i] = from_linear_int(v, a);
    else ((float*)a.out[c])[i] = from_linear(v, a.tf_out, a.p_out, a.kind_out, a.pq_tab);
}

}  // namespace

__global__ __launch_bounds__(256) void k_color_convert(const ColorArgs a) {
    for (int64_t i = blockIdx.x * 256LL + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * 256) {
        float r = linear_sample(a, 0, i);
        if (a.n_planes == 1 && !a.use_matrix && !a.use_tone_map) {  // grey stays grey
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
        if (a.use_tone_map) {  // tone_map_ops.h, in the scale's place
            const ToneMapped o = tone_map_stage(a.tm, r, g, b);
            r = o.r; g = o.g; b = o.b;
        } else if (a.use_scale) {
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
