// The LF image of a VarDCT frame as the picture at 1:8 (JXLDecoder(downsample=8)): every LF group of the frame through the LF stage
// of k_lf.hip -- dequantisation, LF chroma-from-luma, adaptiveSmooth per LF group (LFCoefficients.java:65-180) -- and, for an XYB
// image, OpsinInverseMatrix.invertXYB, written as three planes of ceil(h / 8) x ceil(w / 8) samples in ONE launch.
//
// One lane per cell, 64 x 4 cells per workgroup as in k_lf_dequant. The LF-group pitch is 256 cells, a multiple of the workgroup's
// 64 x 4, so a workgroup lies in one LF group and its group record is read through scalar loads. The cell's arithmetic is
// lf_cell.h's, the pixel's inverse XYB is sample_ops.h's: neither is restated here. Smoothing stops at the LF group's border as the
// reference's does (its border cells are copies), so a seam between two LF groups is two columns (rows) of unsmoothed cells.
#include "lf_cell.h"
#include "lf_image.h"
#include "sample_ops.h"

namespace jxl {

// what lf_cell reads, filled from the workgroup's group record
struct LfGroupCell {
    const int32_t* q[3];
    int H, W;
    float sd[3], sd_gap[3];
    float kX, kB;
    int smooth;
};

__global__ __launch_bounds__(256) void k_lf_image(const LfImageArgs a) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= a.W || y >= a.H) return;
    const LfImageGroup& g = a.groups[(int)((blockIdx.y * 4) >> 8) * a.gcols + (int)((blockIdx.x * 64) >> 8)];
    const int ly = y & 255, lx = x & 255;
    if (ly >= g.H || lx >= g.W) return;  // (the host's validator has the groups tile the grid: never taken)
    LfGroupCell c;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        c.q[i] = a.ints + g.q_off[i];
        c.sd[i] = g.sd[i];
        c.sd_gap[i] = g.sd_gap[i];
    }
    c.H = g.H;
    c.W = g.W;
    c.kX = g.kX;
    c.kB = g.kB;
    c.smooth = g.smooth;
    float o[3];
    lf_cell(c, ly, lx, o);
    if (a.xyb) invert_xyb_px(a.xybp, o[0], o[1], o[2]);
    const int64_t d = (int64_t)y * a.W + x;
#pragma unroll
    for (int i = 0; i < 3; i++) a.out[i][d] = o[i];
}

void launch_lf_image(const LfImageArgs& a, hipStream_t s) {
    if (a.H <= 0 || a.W <= 0) return;
    hipLaunchKernelGGL(k_lf_image, dim3((a.W + 63) / 64, (a.H + 3) / 4), dim3(256), 0, s, a);
}

}  // namespace jxl
