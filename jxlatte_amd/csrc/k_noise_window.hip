// Frame.initializeNoise + synthesizeNoise (Frame.java:748-835) of a whole frame, restricted to a window of it: the stage a
// region decode cannot crop before it runs, because a pixel's noise depends on where the pixel lies in the frame (the group's
// seed, the place in the group's stream, the mirror at the frame's edges). Two launches over NoiseWindowPlan's geometry
// (noise_window_check.h, which also states the bounds both kernels rely on):
//   k_noise_window_rng   XorShiro for exactly the groups the apron touches, seeded with their absolute origin and advanced through
//                        all three channels' rows in the reference's order (:762-772: the channel loop is outermost); only the
//                        samples inside the apron are stored. Lane layout as k_noise_rng (k_post.hip): 8 lanes per group.
//   k_noise_window_add   per window pixel the 5x5 high-pass of the three channels, mirrored against the FRAME's size, then
//                        synthesizeNoise's arithmetic (noise_ops.h).
// Compiled with -ffp-contract=off like every file that holds the reference's arithmetic.
#include <hip/hip_runtime.h>

#include "noise_ops.h"
#include "noise_window.h"

namespace jxl {
namespace {

__device__ __forceinline__ uint64_t split_mix64(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

// lane i of a group's eight owns XorShiro's state0[i] / state1[i] and emits pixels x + 2i, x + 2i + 1 of each run of 16
__global__ __launch_bounds__(64) void k_noise_window_rng(NoiseWindowPlan p, uint64_t seed0, float* __restrict__ o0, float* __restrict__ o1,
                                                         float* __restrict__ o2) {
    const int lane = threadIdx.x & 7;
    const int group = blockIdx.x * 8 + (threadIdx.x >> 3);
    if (group >= p.n_groups) return;
    const int gd = p.group_dim;
    const int y0 = (p.gy0 + group / p.gw) * gd;  // the group's origin in the frame
    const int x0 = (p.gx0 + group % p.gw) * gd;
    const uint64_t seed1 = ((uint64_t)(uint32_t)x0 << 32) | (uint64_t)(uint32_t)y0;
    uint64_t s0 = split_mix64(seed0 + 0x9e3779b97f4a7c15ull);
    uint64_t s1 = split_mix64(seed1 + 0x9e3779b97f4a7c15ull);
    for (int i = 0; i < lane; i++) {
        s0 = split_mix64(s0);
        s1 = split_mix64(s1);
    }
    const int ySize = min(gd, p.frame_h - y0);
    const int xSize = min(gd, p.frame_w - x0);
    const int ay1 = p.ay0 + p.ah, ax1 = p.ax0 + p.aw;
    float* outs[3] = {o0, o1, o2};
    for (int c = 0; c < 3; c++) {
        float* o = outs[c];
        for (int y = 0; y < ySize; y++) {
            const int Y = y0 + y;
            if (c == 2 && Y >= ay1) return;  // nothing behind this point of the stream is stored
            const bool row_in = Y >= p.ay0 && Y < ay1;
            const int64_t row = (int64_t)(Y - p.ay0) * p.aw - p.ax0;  // + the frame's X: inside the apron's plane where row_in and ax0 <= X < ax1
            for (int x = 0; x < xSize; x += 16) {
                const uint64_t a = s1;
                uint64_t b = s0;
                const uint64_t cc = a + b;
                s0 = a;
                b ^= b << 23;
                s1 = b ^ a ^ (b >> 18) ^ (a >> 5);
                const uint32_t lo = (uint32_t)cc, hi = (uint32_t)(cc >> 32);
                const int px = x + 2 * lane, X = x0 + px;
                if (row_in && px < xSize && X >= p.ax0 && X < ax1) o[row + X] = __uint_as_float((lo >> 9) | 0x3f800000u);
                if (row_in && px + 1 < xSize && X + 1 >= p.ax0 && X + 1 < ax1) o[row + X + 1] = __uint_as_float((hi >> 9) | 0x3f800000u);
            }
        }
    }
}

struct NoiseWindowLut {
    float v[8];
};

// one thread per window pixel; n0..n2: the raw noise on the apron (ah x aw), p0..p2: the window's planes (win_h x win_w)
__global__ __launch_bounds__(256) void k_noise_window_add(NoiseWindowPlan p, const float* __restrict__ n0, const float* __restrict__ n1,
                                                          const float* __restrict__ n2, float* p0, float* p1, float* p2, NoiseWindowLut lut,
                                                          float bcx, float bcb) {
    __shared__ float l[8];
    if (threadIdx.x < 8) l[threadIdx.x] = lut.v[threadIdx.x];
    __syncthreads();
    const int64_t n = p.window_floats;
    for (int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int wy = (int)(i / p.win_w), wx = (int)(i - (int64_t)wy * p.win_w);
        const int y = p.y0 + wy, x = p.x0 + wx;  // in the frame
        float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f;
#pragma unroll
        for (int iy = 0; iy < 5; iy++) {
            // (noise_window_apron_holds: the mirrored coordinate lies inside the apron; the clamp costs two instructions and keeps
            // the read inside the allocation whatever the arguments)
            const int cy = min(max(noise_mirror(y + iy - 2, p.frame_h) - p.ay0, 0), p.ah - 1);
#pragma unroll
            for (int ix = 0; ix < 5; ix++) {
                const int cx = min(max(noise_mirror(x + ix - 2, p.frame_w) - p.ax0, 0), p.aw - 1);
                const int64_t at = (int64_t)cy * p.aw + cx;
                const float t = noise_tap(iy, ix);
                a0 += n0[at] * t;
                a1 += n1[at] * t;
                a2 += n2[at] * t;
            }
        }
        float X = p0[i], Y = p1[i], B = p2[i];
        noise_add_px(l, a0, a1, a2, bcx, bcb, X, Y, B);
        p1[i] = Y;
        p0[i] = X;
        p2[i] = B;
    }
}

}  // namespace

void launch_noise_window(const NoiseWindowPlan& p, uint64_t seed0, float* const apron[3], float* const planes[3], const float lut[8],
                         float bcx, float bcb, hipStream_t s) {
    hipLaunchKernelGGL(k_noise_window_rng, dim3((unsigned)((p.n_groups + 7) / 8)), dim3(64), 0, s, p, seed0, apron[0], apron[1], apron[2]);
    NoiseWindowLut l;
    for (int i = 0; i < 8; i++) l.v[i] = lut[i];
    int64_t blocks = (p.window_floats + 255) / 256;
    if (blocks > 65536) blocks = 65536;
    hipLaunchKernelGGL(k_noise_window_add, dim3((unsigned)blocks), dim3(256), 0, s, p, apron[0], apron[1], apron[2], planes[0], planes[1],
                       planes[2], l, bcx, bcb);
}

}  // namespace jxl
