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
#include "jxl_internal.h"
#include "modular_tend.h"

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

}  // namespace

void launch_modplanes(const ModPlanesArgs& p, hipStream_t s) {
    if (p.h <= 0 || p.w <= 0 || p.n <= 0 || p.n > JXL_CANVAS_MAX_PLANES) return;
    int64_t grid = ((((int64_t)p.w + 3) / 4) * p.h + 255) / 256;
    if (grid > 4096) grid = 4096;
    hipLaunchKernelGGL(k_modplanes, dim3((unsigned)grid, (unsigned)p.n), dim3(256), 0, s, p);
}

}  // namespace jxl
