// The Modular context's result channels into the planes of a plane set (Frame.java:430-455 for all output planes at once):
//
//   k_modplanes, per sample of plane i (blockIdx.y):
//     1. crop: row y of the plane is the first `w` samples of row y of its channel, whose pitch is the channel's own width
//     2. int32 plane: the sample as it is; float plane: scale * (float)(a [+ b]) -- the sum wraps (wadd), the conversion rounds
//        first, then ONE f32 multiply: k_modular_to_float's arithmetic (file compiled with -ffp-contract=off like every other)
//   The plane's descriptor is read from the argument block by blockIdx.y, so it is wave-uniform: its branches are scalar.
//
// Shape (k_pfm.hip's): one lane owns 4 consecutive pixels of a row; groups are counted per row, so no lane straddles rows. A
// channel starts kVhPad samples into its allocation and its pitch is any width, a plane's rows are `w` words, unpadded: the
// lane's addresses are only 4-byte aligned, so the vectors are declared with that alignment and the compiler is told the
// truth (gfx950 code objects run with unaligned access enabled: global_load_dwordx4 / global_store_dwordx4). The last group of
// a row whose width is no multiple of 4 loads and stores sample by sample. Plain global loads and stores, 64-bit offsets, no LDS.
//
//   k_modplanes_up<K>, per plane i (blockIdx.y): Frame.performUpsampling (Frame.java:217-260) of castToFloat of the cropped
//   channel, as ONE launch for all planes (jxl_canvas_from_modular_up):
//     1. a tap is sample (ny, nx) of the h x w crop, ny / nx through MathHelper.mirrorCoordinate: scale * (float)(a [+ b]) as above
//     2. the output is k_upsample's (k_post.hip), operation for operation: 25 taps, their window minimum from Float.MAX_VALUE and
//        maximum from Float.MIN_VALUE (kept as the reference has it), the sum from 0f in iy, ix order, the clamp
//   Shape: k_upsample's -- one thread per (input pixel, ky), K contiguous outputs, the K * K * 25 weights in LDS. Every thread
//   converts its own 25 taps (no converted tile in LDS): 25 v_cvt_f32_i32 and 25 more v_mul_f32 per thread, +13 .. 19 % VALU
//   instructions against k_upsample<K>; the int32 taps of neighbouring lanes come from the same cache lines as k_upsample's
//   float ones, and the kernel keeps k_upsample's resource row.
#include "jxl_internal.h"
#include "modular_tend.h"

#include <algorithm>

namespace jxl {
namespace {

typedef uint32_t u32x4a __attribute__((ext_vector_type(4), aligned(4)));

__device__ __forceinline__ uint32_t modplane_word(int32_t v, bool is_float, float scale) {
    return is_float ? __builtin_bit_cast(uint32_t, scale * (float)v) : (uint32_t)v;
}

__global__ __launch_bounds__(256) void k_modplanes(const ModPlanesArgs p) {
    const ModPlane q = p.p[blockIdx.y];
    const bool is_float = q.is_float != 0, add = q.b != nullptr;
    const int64_t gpr = ((int64_t)p.w + 3) >> 2;  // groups per row
    const int64_t groups = gpr * p.h;
    for (int64_t g = blockIdx.x * 256LL + threadIdx.x; g < groups; g += (int64_t)gridDim.x * 256) {
        const int64_t y = g / gpr;
        const int x0 = (int)(g - y * gpr) << 2;
        const int cnt = p.w - x0;  // >= 1
        const int64_t i0 = y * q.pitch + x0;
        uint32_t* o = q.out + y * p.w + x0;
        if (cnt >= 4) {
            u32x4a v = *reinterpret_cast<const u32x4a*>(q.a + i0);
            if (add) {
                const u32x4a u = *reinterpret_cast<const u32x4a*>(q.b + i0);
#pragma unroll
                for (int k = 0; k < 4; k++) v[k] = (uint32_t)wadd((int32_t)v[k], (int32_t)u[k]);
            }
#pragma unroll
            for (int k = 0; k < 4; k++) v[k] = modplane_word((int32_t)v[k], is_float, q.scale);
            *reinterpret_cast<u32x4a*>(o) = v;
        } else {
            for (int k = 0; k < cnt; k++) {
                int32_t v = q.a[i0 + k];
                if (add) v = wadd(v, q.b[i0 + k]);
                o[k] = modplane_word(v, is_float, q.scale);
            }
        }
    }
}

// MathHelper.mirrorCoordinate (MathHelper.java:323-329)
__device__ __forceinline__ int mirror_c(int c, int size) {
    while (c < 0 || c >= size) {
        const int tc = ~c;
        c = tc >= 0 ? tc : (size << 1) + tc;
    }
    return c;
}

template <int K>
__global__ __launch_bounds__(256) void k_modplanes_up(const ModUpArgs p) {
    __shared__ float wl[K * K * 25];
    for (int i = threadIdx.x; i < K * K * 25; i += 256) wl[i] = p.weights[i];
    __syncthreads();
    const ModUpPlane q = p.p[blockIdx.y];
    const bool add = q.b != nullptr;
    const int h = p.h, w = p.w;
    const int64_t n = (int64_t)h * w * K;
    const int64_t ow = (int64_t)w * K;
    for (int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        // i = (y*K + ky) * w + x: consecutive threads walk along an output row
        const int x = (int)(i % w);
        const int64_t oy = i / w;
        const int y = (int)(oy / K), ky = (int)(oy % K);
        float s[25];
        float mn = 3.4028234663852886e38f;
        float mx = 1.4e-45f;  // Float.MIN_VALUE (Frame.java:241), not -MAX_VALUE: kept as the reference has it
#pragma unroll
        for (int iy = 0; iy < 5; iy++) {
            const int64_t row = (int64_t)mirror_c(y + iy - 2, h) * q.pitch;
#pragma unroll
            for (int ix = 0; ix < 5; ix++) {
                const int64_t at = row + mirror_c(x + ix - 2, w);
                int32_t t = q.a[at];
                if (add) t = wadd(t, q.b[at]);
                const float v = q.scale * (float)t;
                s[iy * 5 + ix] = v;
                if (v < mn) mn = v;
                if (v > mx) mx = v;
            }
        }
        float* o = q.out + oy * ow + (int64_t)x * K;
#pragma unroll
        for (int kx = 0; kx < K; kx++) {
            const float* wt = wl + (ky * K + kx) * 25;
            float total = 0.0f;
#pragma unroll
            for (int t = 0; t < 25; t++) total += wt[t] * s[t];
            o[kx] = total < mn ? mn : total > mx ? mx : total;
        }
    }
}

}  // namespace

void launch_modplanes_up(const ModUpArgs& p, int k, hipStream_t s) {
    if (p.h <= 0 || p.w <= 0 || p.n <= 0 || p.n > JXL_CANVAS_MAX_PLANES || !p.weights) return;
    const dim3 g((unsigned)std::min<int64_t>(((int64_t)p.h * p.w * k + 255) / 256, 4096), (unsigned)p.n);
    if (k == 2) hipLaunchKernelGGL(k_modplanes_up<2>, g, dim3(256), 0, s, p);
    else if (k == 4) hipLaunchKernelGGL(k_modplanes_up<4>, g, dim3(256), 0, s, p);
    else if (k == 8) hipLaunchKernelGGL(k_modplanes_up<8>, g, dim3(256), 0, s, p);
}

void launch_modplanes(const ModPlanesArgs& p, hipStream_t s) {
    if (p.h <= 0 || p.w <= 0 || p.n <= 0 || p.n > JXL_CANVAS_MAX_PLANES) return;
    int64_t grid = ((((int64_t)p.w + 3) / 4) * p.h + 255) / 256;
    if (grid > 4096) grid = 4096;
    hipLaunchKernelGGL(k_modplanes, dim3((unsigned)grid, (unsigned)p.n), dim3(256), 0, s, p);
}

}  // namespace jxl
