// The varblock map drawn onto the picture (Frame.drawVarblocks, Frame.java:464-503): every varblock of a VarDCT frame tinted by
// its transform type, its top row and left column black.
//
//   k_varblocks, per pixel (y, x) of the planes:
//     1. the cell (y >> 3, x >> 3) of the host-built map (varblock_check.h): outside the cell grid, or 0xFF (no block): untouched
//     2. a border pixel -- (y & 7) == 0 in a cell of its block's top cell row (bit 5), or (x & 7) == 0 in a cell of its block's
//        left cell column (bit 6) -- becomes 0f in all three planes (:488-491)
//     3. else light = 0.25f * (R + B) + 0.5f * G; light = (float)Math.cbrt(light) * 0.5f + 0.25f;
//        out_c = factor_c * 0.5f + 0.5f * sample_c / light (:493-497), every product, sum and quotient rounded on its own (file
//        compiled with -ffp-contract=off like every other); the division is the IEEE one; cbrt is the double-precision one of
//        the device library on the float widened to double, its result cast back. factor_c comes from the 27 x 3 table the host
//        computes (:476-479); factor_c * 0.5f is made once per lane (the same single rounding).
//   A zero or negative light gives what IEEE gives (infinities, NaN).
//
// Shape (k_pfm.hip's): one lane owns 4 consecutive pixels of a row, groups counted per row, so a group starts at a multiple of 4
// and lies inside ONE cell: one map byte per lane. A 16-byte load and a 16-byte store per plane, in place; rows are W floats,
// unpadded, so unless W is a multiple of 4 the addresses are only 4-byte aligned and the vectors are declared with that alignment
// (f32x4a). The last group of a row whose width is no multiple of 4 goes sample by sample. Plain global loads and stores, no
// LDS, 64-bit offsets.
#include "jxl_internal.h"

namespace jxl {
namespace {

typedef float f32x4a __attribute__((ext_vector_type(4), aligned(4)));

// one pixel that is no border pixel; h0..h2 = factor_c * 0.5f
__device__ __forceinline__ void vb_tint(float& r, float& g, float& b, float h0, float h1, float h2) {
    float light = 0.25f * (r + b) + 0.5f * g;
    light = (float)cbrt((double)light) * 0.5f + 0.25f;
    r = h0 + (0.5f * r) / light;
    g = h1 + (0.5f * g) / light;
    b = h2 + (0.5f * b) / light;
}

__global__ __launch_bounds__(256) void k_varblocks(const VarblockArgs p) {
    const int64_t gpr = ((int64_t)p.w + 3) >> 2;  // groups per row
    const int64_t groups = gpr * p.h;
    for (int64_t gi = blockIdx.x * 256LL + threadIdx.x; gi < groups; gi += (int64_t)gridDim.x * 256) {
        const int64_t y = gi / gpr;
        const int x0 = (int)(gi - y * gpr) << 2;
        const int cy = (int)(y >> 3), cx = x0 >> 3;
        if (cy >= p.cells_h || cx >= p.cells_w) continue;
        const uint32_t m = p.map[(int64_t)cy * p.cells_w + cx];
        if (m == 0xffu) continue;
        const float* f = p.factors + 3 * (m & 0x1fu);
        const float h0 = f[0] * 0.5f, h1 = f[1] * 0.5f, h2 = f[2] * 0.5f;
        const bool top = (m & 0x20u) && (y & 7) == 0;
        const bool left = (m & 0x40u) && (x0 & 7) == 0;  // of the group's first pixel: the other three have x & 7 != 0
        const int cnt = p.w - x0;                        // >= 1
        const int64_t i0 = y * p.w + x0;
        if (cnt >= 4) {
            f32x4a* a0 = reinterpret_cast<f32x4a*>(p.pl[0] + i0);
            f32x4a* a1 = reinterpret_cast<f32x4a*>(p.pl[1] + i0);
            f32x4a* a2 = reinterpret_cast<f32x4a*>(p.pl[2] + i0);
            f32x4a r = *a0, g = *a1, b = *a2;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                float rr = r[k], gg = g[k], bb = b[k];
                if (top || (left && k == 0)) rr = gg = bb = 0.0f;
                else vb_tint(rr, gg, bb, h0, h1, h2);
                r[k] = rr; g[k] = gg; b[k] = bb;
            }
            *a0 = r;
            *a1 = g;
            *a2 = b;
        } else {
            for (int k = 0; k < cnt; k++) {
                float rr = p.pl[0][i0 + k], gg = p.pl[1][i0 + k], bb = p.pl[2][i0 + k];
                if (top || (left && k == 0)) rr = gg = bb = 0.0f;
                else vb_tint(rr, gg, bb, h0, h1, h2);
                p.pl[0][i0 + k] = rr;
                p.pl[1][i0 + k] = gg;
                p.pl[2][i0 + k] = bb;
            }
        }
    }
}

}  // namespace

void launch_varblocks(const VarblockArgs& p, hipStream_t s) {
    if (p.h <= 0 || p.w <= 0 || p.cells_h <= 0 || p.cells_w <= 0) return;
    int64_t grid = ((((int64_t)p.w + 3) / 4) * p.h + 255) / 256;
    if (grid > 16384) grid = 16384;
    hipLaunchKernelGGL(k_varblocks, dim3((unsigned)grid), dim3(256), 0, s, p);
}

}  // namespace jxl
