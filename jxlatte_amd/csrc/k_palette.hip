// The inverse Palette transform of the frame-level Modular stream (ModularStream.java:327-378), on planes in device memory. The
// per-sample arithmetic is palette_ops.h's; what jxl_stage_palette has let through (palette_check.h) makes every read below safe
// without a clamp.
//
//   k_palette_lookup, grid-stride over groups of 4 consecutive samples of the index plane (the planes are flat here: a group may
//   span two rows). A lane reads its 4 indices once (one 16-byte load; the planes start 16-byte aligned and a group starts at a
//   multiple of 4) and writes all num_c outputs, one 16-byte store per plane; the last group of a plane whose size is no
//   multiple of 4 goes sample by sample. The num_c x nb_colors palette is staged in LDS when it has at most kPaletteLdsInts
//   entries, else it is read from global memory (the instantiation is picked by the launcher). Its rows lie pal_pitch apart:
//   back to back from jxl_stage_palette, the palette channel's own width in a plan of jxl_modular_begin_chain.
//     A pixel with index < nb_deltas (a "delta pixel") is value + prediction (:368-369). For d_pred 0 the prediction is 0 and for
//   d_pred 6 it is (pred + 3) >> 3 of the weighted predictor's plane (0 without one): neither reads a neighbour, so both finish
//   here. For every other predictor the kernel writes the value alone. It counts the delta pixels either way: a wave sums its
//   lanes' counts by shuffles, the waves add theirs in LDS, and one lane makes ONE vector atomic add per workgroup to the
//   device counter.
//
//   k_palette_chain runs only when that count is not zero and d_pred is neither 0 nor 6. A delta pixel adds the prediction made
//   from the OUTPUTS of its causal neighbours (ModularChannel.java:95-121, 143-183), the farthest being (x + 2, y - 1); every one
//   of them has a smaller t = x + 3 * y. One workgroup per output plane (the planes are independent) walks t = 0 .. w + 3 * h - 4;
//   its lanes take the pixels (t - 3 * y, y) of that t, kPaletteChainThreads rows apart, and skip those that are no delta pixel.
//   One __syncthreads() per step, behind an explicit s_waitcnt vmcnt(0): every wave's stores of the step have completed before
//   it joins the barrier, and no lane of the workgroup -- the same CU, the same write-through L1 -- loads them before it leaves
//   it. (hipcc lowers the workgroup-scope fences of __syncthreads() to a bare s_barrier here, relying on the CU's vector memory
//   path keeping the order of its requests; the wait makes the hand-off independent of that and costs nothing next to the
//   loads the next step waits for anyway.) The trip count is fixed by the shape: no flag, no spin, no wait between workgroups,
//   no persistent grid. Its cost is a barrier and a round trip to memory per step, however few delta pixels there are; delta
//   palettes are libjxl's opt-in lossy-palette mode (profiles/device_palette.md has the times).
#include "jxl_internal.h"
#include "palette_ops.h"

namespace jxl {
namespace {

typedef int32_t i32x4 __attribute__((ext_vector_type(4)));

template <bool kLds>
__global__ __launch_bounds__(256) void k_palette_lookup(const PaletteArgs p) {
    extern __shared__ int32_t s_pal[];
    __shared__ unsigned int s_count;
    if (threadIdx.x == 0) s_count = 0;
    if (kLds) {
        if (p.pal_pitch == p.nb_colors) {
            const int entries = p.num_c * p.nb_colors;  // <= kPaletteLdsInts
            for (int j = threadIdx.x; j < entries; j += 256) s_pal[j] = p.palette[j];
        } else {  // a plan's palette channel is wider than nb_colors: row by row
            for (int c = 0; c < p.num_c; c++)
                for (int j = threadIdx.x; j < p.nb_colors; j += 256) s_pal[c * p.nb_colors + j] = p.palette[(int64_t)c * p.pal_pitch + j];
        }
    }
    __syncthreads();
    PaletteLookup lk;
    lk.palette = kLds ? s_pal : p.palette;
    lk.pal_w = kLds ? p.nb_colors : p.pal_pitch;  // the rows stand back to back in LDS
    lk.nb_colors = p.nb_colors;
    lk.bit_depth = p.bit_depth;
    const int64_t n = (int64_t)p.h * p.w;
    const int64_t groups = (n + 3) >> 2;
    const bool wp = p.d_pred == 6 && p.pred != nullptr;
    unsigned int deltas = 0;
    for (int64_t gi = blockIdx.x * 256LL + threadIdx.x; gi < groups; gi += (int64_t)gridDim.x * 256) {
        const int64_t i0 = gi << 2;
        if (i0 + 4 <= n) {
            const i32x4 idx = *reinterpret_cast<const i32x4*>(p.index + i0);
            i32x4 add = {0, 0, 0, 0};
            if (wp) {
                const i32x4 pr = *reinterpret_cast<const i32x4*>(p.pred + i0);
#pragma unroll
                for (int k = 0; k < 4; k++) add[k] = idx[k] < p.nb_deltas ? palette_predict_wp(pr[k]) : 0;
            }
#pragma unroll
            for (int k = 0; k < 4; k++) deltas += idx[k] < p.nb_deltas;
            for (int c = 0; c < p.num_c; c++) {
                i32x4 v;
#pragma unroll
                for (int k = 0; k < 4; k++) v[k] = jadd(palette_value(idx[k], c, lk), add[k]);
                *reinterpret_cast<i32x4*>(p.out + c * p.plane_stride + i0) = v;
            }
        } else {
            for (int64_t i = i0; i < n; i++) {
                const int32_t idx = p.index[i];
                const bool is_delta = idx < p.nb_deltas;
                const int32_t add = wp && is_delta ? palette_predict_wp(p.pred[i]) : 0;
                deltas += is_delta;
                for (int c = 0; c < p.num_c; c++) p.out[c * p.plane_stride + i] = jadd(palette_value(idx, c, lk), add);
            }
        }
    }
    for (int off = 32; off > 0; off >>= 1) deltas += __shfl_down(deltas, off, 64);
    if ((threadIdx.x & 63) == 0 && deltas) atomicAdd(&s_count, deltas);
    __syncthreads();
    if (threadIdx.x == 0 && s_count) atomicAdd(p.delta_count, s_count);
}

__global__ __launch_bounds__(kPaletteChainThreads) void k_palette_chain(const PaletteArgs p) {
    int32_t* o = p.out + blockIdx.x * p.plane_stride;
    const int64_t steps = (int64_t)p.w + 3 * (int64_t)p.h - 3;  // t = 0 .. (w - 1) + 3 * (h - 1)
    for (int64_t t = 0; t < steps; t++) {
        // the pixels of this t: x = t - 3 * y with 0 <= x < w and 0 <= y < h
        const int64_t y_lo = t >= p.w ? (t - p.w + 3) / 3 : 0;  // ceil((t - (w - 1)) / 3)
        const int64_t y_top = t / 3;
        const int64_t y_hi = y_top < p.h - 1 ? y_top : p.h - 1;
        for (int64_t y = y_lo + threadIdx.x; y <= y_hi; y += kPaletteChainThreads) {
            const int32_t x = (int32_t)(t - 3 * y);
            const int64_t i = y * p.w + x;
            if (p.index[i] < p.nb_deltas) o[i] = jadd(o[i], palette_predict_at(p.d_pred, o, p.w, x, (int32_t)y));
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's stores of the step have completed ...
        __syncthreads();                                  // ... before any wave of the workgroup starts the next step
    }
}

}  // namespace

void launch_palette_lookup(const PaletteArgs& p, hipStream_t s) {
    if (p.h <= 0 || p.w <= 0 || p.num_c <= 0) return;
    const int64_t groups = ((int64_t)p.h * p.w + 3) / 4;
    int64_t grid = (groups + 255) / 256;
    if (grid > 4096) grid = 4096;
    const int64_t entries = (int64_t)p.num_c * p.nb_colors;
    if (entries <= kPaletteLdsInts)
        hipLaunchKernelGGL(k_palette_lookup<true>, dim3((unsigned)grid), dim3(256), sizeof(int32_t) * (size_t)entries, s, p);
    else
        hipLaunchKernelGGL(k_palette_lookup<false>, dim3((unsigned)grid), dim3(256), 0, s, p);
}

void launch_palette_chain(const PaletteArgs& p, hipStream_t s) {
    if (p.h <= 0 || p.w <= 0 || p.num_c <= 0) return;
    hipLaunchKernelGGL(k_palette_chain, dim3((unsigned)p.num_c), dim3(kPaletteChainThreads), 0, s, p);
}

}  // namespace jxl
