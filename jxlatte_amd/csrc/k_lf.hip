// LF stage on gfx950 (row f1 of the scope table): LF dequantisation + LF chroma-from-luma + adaptive LF smoothing
// of one LF group, written straight into the frame-level LF planes the IDCT stage reads.
//
// Replaces J/frame/vardct/LFCoefficients.java:65-75 (dequant), :78-95 (chroma from luma), :113-180 (adaptiveSmooth).
// lfIndex (:105-111,182-…) feeds the entropy decoder's context model and stays on the host.
//
// One lane per 8x8 cell; the cell's arithmetic is lf_cell.h's (shared with k_lf_image.hip). 1/64 of the frame's pixels, the
// kernel is a few microseconds.
#include "jxl_internal.h"
#include "lf_cell.h"

namespace jxl {

struct LfArgs {
    const int32_t* q[3];   // lfQuant in X,Y,B order, [H][W] of the LF group
    float* out[3];         // frame-level LF planes
    int H, W;              // LF group size in cells
    int64_t out_off;       // offset of the LF group's (0,0) cell in the frame-level plane
    int out_stride;        // frame-level plane row stride (cells)
    float sd[3];           // scaledDequant[i] / (1 << extraPrecision)
    float sd_gap[3];       // scaledDequant[i]
    float kX, kB;
    int smooth;
};

__global__ __launch_bounds__(256) void k_lf_dequant(const LfArgs a) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= a.W || y >= a.H) return;
    float o[3];
    lf_cell(a, y, x, o);  // lf_cell.h: dequant, chroma from luma, adaptiveSmooth (border cells are copied)
    const int64_t d = a.out_off + (int64_t)y * a.out_stride + x;
#pragma unroll
    for (int i = 0; i < 3; i++) a.out[i][d] = o[i];
}

__global__ __launch_bounds__(256) void k_lf_dequant_plain(const int32_t* __restrict__ q, float* __restrict__ out, int H, int W,
                                                          int64_t out_off, int out_stride, float sd) {
    const int n = H * W;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const int y = i / W, x = i - y * W;
        out[out_off + (int64_t)y * out_stride + x] = (float)q[i] * sd;  // LFCoefficients.java:66-75
    }
}

void launch_lf_dequant_plain(const int32_t* q, float* out, int H, int W, int64_t out_off, int out_stride, float scaled_dequant,
                             int extra_precision, hipStream_t s) {
    if (H <= 0 || W <= 0) return;
    const float sd = scaled_dequant / (float)(1 << extra_precision);
    const int grid = std::min(4096, (H * W + 255) / 256);
    hipLaunchKernelGGL(k_lf_dequant_plain, dim3(grid), dim3(256), 0, s, q, out, H, W, out_off, out_stride, sd);
}

void launch_lf_dequant(const int32_t* const q[3], float* const out[3], int H, int W, int64_t out_off, int out_stride,
                       const float scaled_dequant[3], int extra_precision, float base_corr_x, float base_corr_b,
                       int color_factor, int x_factor_lf, int b_factor_lf, int smooth, hipStream_t s) {
    if (H <= 0 || W <= 0) return;
    LfArgs a;
    for (int i = 0; i < 3; i++) {
        a.q[i] = q[i];
        a.out[i] = out[i];
        a.sd[i] = scaled_dequant[i] / (float)(1 << extra_precision);  // LFCoefficients.java:69
        a.sd_gap[i] = scaled_dequant[i];
    }
    a.H = H;
    a.W = W;
    a.out_off = out_off;
    a.out_stride = out_stride;
    // SPEC: -128, not -127 (LFCoefficients.java:80-82)
    a.kX = base_corr_x + ((float)x_factor_lf - 128.0f) / (float)color_factor;
    a.kB = base_corr_b + ((float)b_factor_lf - 128.0f) / (float)color_factor;
    a.smooth = smooth;
    hipLaunchKernelGGL(k_lf_dequant, dim3((W + 63) / 64, (H + 3) / 4), dim3(256), 0, s, a);
}

}  // namespace jxl
