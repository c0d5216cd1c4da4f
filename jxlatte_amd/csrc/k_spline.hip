// Frame.renderSplines / Spline.renderSpline (J/frame/features/spline/Spline.java:180-197) as a pixel-owned gather.
// One workgroup = one non-empty 32 x 8 tile of the host's binning (spline_host.hip), one lane = one pixel, one wave = two rows
// of 32. A lane loads its three samples, walks the tile's arc list IN TABLE ORDER, adds the three terms of every arc whose box
// holds its pixel to three register accumulators -- the reference's `fby[x] += extra`, arcs in order, one += per arc and
// channel -- and stores once: no atomics, the same bits on every run. A pixel outside an arc's box adds nothing (not +0.0f:
// a -0.0f sample survives). Every operation is the reference's float operation (no contraction, correctly rounded division
// and square root) except (float)Math.exp(double) (MathHelper.java:53, :61): fp_exp, jxl_fastpow.h.
// The list index and the arc record are wave-uniform: they come through scalar loads (the index depends on blockIdx and the
// loop counter only; the tables are const __restrict__), and an arc whose rows miss the wave's two rows is skipped by a scalar
// branch -- only the box test inside a wave diverges.
#include "jxl_internal.h"
#include "jxl_fastpow.h"

namespace jxl {
namespace {

// MathHelper.erf (MathHelper.java:40-66)
__device__ __forceinline__ float spline_erf(float z) {
    const float az = __builtin_fabsf(z);
    const float nzz = -z * z;
    float m, arg;
    if (az > 1e-4f) {
        const float t = 1.0f / (az * 0.5f + 1.0f);
        const float u = t * (t * (t * (t * (t * (t * (t * (t * (t * 0.17087277f - 0.82215223f) + 1.48851587f) - 1.13520398f)
                          + 0.27886807f) - 0.18628806f) + 0.09678418f) + 0.37409196f) + 1.00002368f) - 1.26551223f;
        m = t;
        arg = nzz + u;
    } else {  // (NaN comes here too, as in the reference)
        const float t = 1.0f / (az * 0.47047f + 1.0f);
        m = t * (t * (t * 0.7478556f - 0.0958798f) + 0.3480242f);
        arg = nzz;
    }
    const float abs_erf = 1.0f - m * (float)fp_exp((double)arg);
    return z < 0 ? -abs_erf : abs_erf;
}

}  // namespace

__global__ __launch_bounds__(256) void k_splines(float* __restrict__ p0, float* __restrict__ p1, float* __restrict__ p2, int h, int w,
                                                 const jxl_spline_arc* __restrict__ arcs, const int32_t* __restrict__ tile,
                                                 const int32_t* __restrict__ start, const int32_t* __restrict__ list, int tiles_x) {
    const float sqrt_f = 0.35355338f;  // MathHelper.SQRT_F = (float)sqrt(0.125)
    const int t = tile[blockIdx.x];
    const int ty = t / tiles_x, tx = t - ty * tiles_x;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    const int wy0 = ty * kSplineTileH + wave * 2;  // the wave's two rows: wy0, wy0 + 1
    const int x = tx * kSplineTileW + (lane & 31), y = wy0 + (lane >> 5);
    const bool inside = x < w && y < h;
    const int64_t at = (int64_t)y * w + x;
    float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f;
    if (inside) {
        a0 = p0[at];
        a1 = p1[at];
        a2 = p2[at];
    }
    const float fy = (float)y, fx = (float)x;
    const int end = start[blockIdx.x + 1];
    for (int i = start[blockIdx.x]; i < end; i++) {
        const jxl_spline_arc a = arcs[list[i]];
        if (a.y1 < wy0 || a.y0 > wy0 + 1) continue;  // wave-uniform
        if (x >= a.x0 && x <= a.x1 && y >= a.y0 && y <= a.y1) {  // (the boxes are clamped to the frame: such a pixel is inside)
            const float dy = fy - a.y, dx = fx - a.x;
            const float distance = __builtin_sqrtf(dy * dy + dx * dx);  // (float)Math.sqrt((double)float): the same value
            float factor = spline_erf((0.5f * distance + sqrt_f) * a.inv_sigma);
            factor -= spline_erf((0.5f * distance - sqrt_f) * a.inv_sigma);
            a0 += a.mul[0] * factor * factor;
            a1 += a.mul[1] * factor * factor;
            a2 += a.mul[2] * factor * factor;
        }
    }
    if (inside) {
        p0[at] = a0;
        p1[at] = a1;
        p2[at] = a2;
    }
}

void launch_splines(float* const planes[3], int h, int w, const jxl_spline_arc* arcs, const int32_t* tile, const int32_t* start,
                    const int32_t* list, int n_tiles, int tiles_x, hipStream_t s) {
    if (n_tiles <= 0) return;
    hipLaunchKernelGGL(k_splines, dim3((unsigned)n_tiles), dim3(256), 0, s, planes[0], planes[1], planes[2], h, w, arcs, tile, start, list,
                       tiles_x);
}

}  // namespace jxl
