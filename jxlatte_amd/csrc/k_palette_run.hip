// A run of consecutive inverse Palette transforms of the frame-level Modular chain (ModularStream.java:327-378) as ONE launch.
// While no pixel of the run needs a neighbour, every output plane of the run is a function of one input channel alone: the
// index goes through at most kPalRunMaxDepth lookups, each a (stage, row) pair -- stage k's value is stage k + 1's index, any
// int32 (negative, past nb_colors, INT32_MIN: palette_value of palette_ops.h takes them all, and nothing else computes here).
// modchain_check.h builds the table; jxl_modular_begin_chain (host.hip) lets a run through only when its palettes together have
// at most kPaletteRunLdsInts entries and it has at most kPalRunMaxOut outputs.
//
//   k_palette_run follows k_palette_lookup's shape: grid-stride over groups of 4 consecutive samples of the source plane, one
//   16-byte load per group, one 16-byte store per output plane (every plane of a plan starts 16-byte aligned), the last group
//   of a sample count that is no multiple of 4 sample by sample. All palettes of the run are staged in LDS back to back (row c
//   of stage s at lds_off[s] + c * nb_colors), read from the device copies of the palette channels at their own pitch.
//     The run is exact only if no pixel is a delta pixel (index < nb_deltas at that stage; every negative index is one) of a
//   stage whose predictor reads neighbours (d_pred other than 0 and 6: PaletteRunStage::chained). The kernel counts those over
//   all stages and outputs: a wave sums its lanes' counts by shuffles, the waves add theirs in LDS, one lane makes one vector
//   atomic add per workgroup. A count that is not zero makes the plan run the run again stage by stage (k_palette.hip), where
//   k_palette_chain adds the predictions; what this kernel wrote is then overwritten.
#include "jxl_internal.h"
#include "palette_ops.h"

namespace jxl {
namespace {

typedef int32_t i32x4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(256) void k_palette_run(const PaletteRunArgs p) {
    extern __shared__ int32_t s_pal[];
    __shared__ unsigned int s_count;
    if (threadIdx.x == 0) s_count = 0;
    for (int s = 0; s < p.n_stage; s++) {
        const PaletteRunStage& st = p.st[s];
        for (int c = 0; c < st.num_c; c++)
            for (int j = threadIdx.x; j < st.nb_colors; j += 256) s_pal[st.lds_off + c * st.nb_colors + j] = st.palette[(int64_t)c * st.pal_w + j];
    }
    __syncthreads();
    const int64_t n = p.n;
    const int64_t groups = (n + 3) >> 2;
    unsigned int impure = 0;
    for (int64_t gi = blockIdx.x * 256LL + threadIdx.x; gi < groups; gi += (int64_t)gridDim.x * 256) {
        const int64_t i0 = gi << 2;
        if (i0 + 4 <= n) {
            const i32x4 idx = *reinterpret_cast<const i32x4*>(p.src + i0);
            for (int o = 0; o < p.n_out; o++) {
                const PaletteRunOut& po = p.out[o];
                i32x4 v = idx;
                for (int d = 0; d < po.depth; d++) {
                    const PaletteRunStage& st = p.st[po.stage[d]];
                    PaletteLookup lk;
                    lk.palette = s_pal + st.lds_off;
                    lk.pal_w = st.nb_colors;
                    lk.nb_colors = st.nb_colors;
                    lk.bit_depth = p.bit_depth;
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        impure += (v[k] < st.nb_deltas) & st.chained;
                        v[k] = palette_value(v[k], po.row[d], lk);
                    }
                }
                *reinterpret_cast<i32x4*>(po.plane + i0) = v;
            }
        } else {
            for (int64_t i = i0; i < n; i++) {
                const int32_t idx = p.src[i];
                for (int o = 0; o < p.n_out; o++) {
                    const PaletteRunOut& po = p.out[o];
                    int32_t v = idx;
                    for (int d = 0; d < po.depth; d++) {
                        const PaletteRunStage& st = p.st[po.stage[d]];
                        PaletteLookup lk;
                        lk.palette = s_pal + st.lds_off;
                        lk.pal_w = st.nb_colors;
                        lk.nb_colors = st.nb_colors;
                        lk.bit_depth = p.bit_depth;
                        impure += (v < st.nb_deltas) & st.chained;
                        v = palette_value(v, po.row[d], lk);
                    }
                    po.plane[i] = v;
                }
            }
        }
    }
    for (int off = 32; off > 0; off >>= 1) impure += __shfl_down(impure, off, 64);
    if ((threadIdx.x & 63) == 0 && impure) atomicAdd(&s_count, impure);
    __syncthreads();
    if (threadIdx.x == 0 && s_count) atomicAdd(p.impure, 1u);  // (workgroups with any: a sum of pixels could wrap to 0)
}

}  // namespace

void launch_palette_run(const PaletteRunArgs& p, hipStream_t s) {
    if (p.n <= 0 || p.n_out <= 0) return;
    const int64_t groups = (p.n + 3) / 4;
    int64_t grid = (groups + 255) / 256;
    if (grid > kPaletteRunMaxGrid) grid = kPaletteRunMaxGrid;
    hipLaunchKernelGGL(k_palette_run, dim3((unsigned)grid), dim3(256), sizeof(int32_t) * (size_t)p.lds_ints, s, p);
}

}  // namespace jxl
