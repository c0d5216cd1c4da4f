// JXLCodestreamDecoder.blendFrame (JXLCodestreamDecoder.java:515-537) on device plane sets: ONE launch over every canvas
// channel. The per-sample expressions are jxl_blend.h's (k_blend and k_patches evaluate the same ones); the copy and the int
// ADD of :287-301 are the only functions int32 planes take. File compiled with -ffp-contract=off like every other.
//
// Shape: a lane owns up to 4 consecutive canvas pixels of one row and walks the channels IN CANVAS ORDER, its loads and stores
// in program order. That order is what makes the in-place case right: when the reference set is the canvas set every sample a
// lane reads from it lies at a pixel the lane itself owns (canvas_check.h refuses anything else), so channel c sees what this
// launch stored for the channels before it -- an already blended alpha plane included -- exactly as the reference does when
// reference[k] and canvas are one ImageBuffer[] (:657). No pointer is __restrict__: the compiler keeps a channel's loads behind
// the stores of the channel before. Lanes never share a pixel, so there is no ordering between lanes to keep.
//
// Groups are counted per row and start where the CANVAS address is a multiple of 16 bytes: group 0 of a row takes the 0..3
// samples in front of that boundary, the last group what is left, both sample by sample; every full group stores 16 aligned
// bytes per channel. Frame and reference rows start wherever their own offset puts them: their 16-byte loads are declared
// 4-byte aligned (gfx950 code objects run with unaligned access enabled; global_load_dwordx4 either way). Plain global loads
// and stores only. The function of a channel is a kernel argument: scalar branches, one instance of the kernel.
//
// k_canvas_cast, further down: the whole-plane casts in front of such a launch (and of k_patches on plane sets), all in one.
#include <hip/hip_runtime.h>

#include "jxl_internal.h"
#include "jxl_blend.h"
#include "sample_ops.h"

namespace jxl {
namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4a __attribute__((ext_vector_type(4), aligned(4)));

__device__ __forceinline__ float as_f(uint32_t v) { return __builtin_bit_cast(float, v); }
__device__ __forceinline__ uint32_t as_u(float v) { return __builtin_bit_cast(uint32_t, v); }

// one sample of one channel: blendBuffers' inner switch (:493-512) with the operand order of k_blend
__device__ __forceinline__ uint32_t canvas_sample(int op, int flags, uint32_t f, uint32_t r, float fa, float ra) {
    const bool clamp = flags & JXL_BLEND_FLAG_CLAMP;
    switch (op) {
        case OP_COPY_FRAME: return f;                                 // copyToCanvas (:26-40)
        case OP_COPY_REF: return r;                                   // blendMulAdd on the alpha channel itself (:388-391)
        case OP_ADD_I: return r + f;                                  // :287-301, Java int wrap
        case OP_ADD_F: return as_u(as_f(r) + as_f(f));                // :302-317
        case OP_MULT: return as_u(blend_mult(as_f(f), as_f(r), clamp));
        case OP_BLEND:
            return as_u(blend_blend(as_f(f), as_f(r), fa, ra, (flags & JXL_BLEND_FLAG_IS_ALPHA) != 0, (flags & JXL_BLEND_FLAG_PREMULT) != 0, clamp));
        default: return as_u(blend_muladd(as_f(f), as_f(r), fa, clamp));
    }
}

__global__ __launch_bounds__(256) void k_canvas_blend(const CanvasArgs a) {
    const int gpr = ((a.w + 3) >> 2) + 1;  // groups per row: the samples in front of the first 16-byte boundary, then fours
    const int64_t groups = (int64_t)gpr * a.h;
    for (int64_t g = blockIdx.x * 256LL + threadIdx.x; g < groups; g += (int64_t)gridDim.x * 256) {
        const int y = (int)(g / gpr), j = (int)(g - (int64_t)y * gpr);
        const int lead = (int)((0u - ((uint32_t)a.c_align + (uint32_t)y * (uint32_t)a.cw)) & 3u);
        const int x0 = j == 0 ? 0 : lead + ((j - 1) << 2);
        const int cnt = j == 0 ? (lead < a.w ? lead : a.w) : (a.w - x0 < 4 ? a.w - x0 : 4);
        if (cnt <= 0) continue;
        const int64_t ci = (int64_t)y * a.cw + x0, fi = (int64_t)y * a.fw + x0, ri = (int64_t)y * a.rw + x0;
        for (int c = 0; c < a.n; c++) {
            const CanvasChan& k = a.ch[c];
            const int op = k.op, flags = k.flags;
            if (cnt == 4) {
                u32x4 f = {0, 0, 0, 0}, r = {0, 0, 0, 0}, fa = {0, 0, 0, 0}, ra = {0, 0, 0, 0}, o;
                if (k.frame) f = *reinterpret_cast<const u32x4a*>(k.frame + fi);
                if (k.ref) r = *reinterpret_cast<const u32x4a*>(k.ref + ri);
                if (k.frame_alpha) fa = *reinterpret_cast<const u32x4a*>(k.frame_alpha + fi);
                if (k.ref_alpha) ra = *reinterpret_cast<const u32x4a*>(k.ref_alpha + ri);
#pragma unroll
                for (int i = 0; i < 4; i++) o[i] = canvas_sample(op, flags, f[i], r[i], as_f(fa[i]), as_f(ra[i]));
                *reinterpret_cast<u32x4*>(k.canvas + ci) = o;
            } else {
                for (int i = 0; i < cnt; i++) {
                    const uint32_t f = k.frame ? k.frame[fi + i] : 0u, r = k.ref ? k.ref[ri + i] : 0u;
                    const float fa = k.frame_alpha ? as_f(k.frame_alpha[fi + i]) : 0.0f, ra = k.ref_alpha ? as_f(k.ref_alpha[ri + i]) : 0.0f;
                    k.canvas[ci + i] = canvas_sample(op, flags, f, r, fa, ra);
                }
            }
        }
    }
}

// jxl_canvas_cast_planes: ImageBuffer.castToFloat0 (ImageBuffer.java:112-127) of up to kCastMaxItems whole planes in place, ONE
// launch. A workgroup owns one run of kCastRun consecutive samples of one plane; which plane follows from blockIdx.x and the
// prefix first_block[] alone, so the item record is wave-uniform (scalar loads from the kernel argument). Inside the run: the
// 0..3 samples in front of the first 16-byte boundary and the 0..3 behind the last one go sample by sample, everything between
// as 16-byte loads and stores (a set's planes start 256-byte aligned, so for them only the last run of a plane has a tail).
// Every lane loads exactly the words it stores, so in place is safe without any ordering between lanes.
__global__ __launch_bounds__(256) void k_canvas_cast(const CastArgs a) {
    const int blk = (int)blockIdx.x;
    int item = 0;
    while (item + 1 < a.n && blk >= a.first_block[item + 1]) item++;  // wave-uniform
    const CastItem it = a.it[item];
    const int64_t s = (int64_t)(blk - a.first_block[item]) * kCastRun;
    const int len = (int)(it.n - s < kCastRun ? it.n - s : kCastRun);
    uint32_t* p = it.base + s;
    const int t = (int)threadIdx.x;
    int lead = (int)((0u - (uint32_t)(reinterpret_cast<uintptr_t>(p) >> 2)) & 3u);
    if (lead > len) lead = len;
    if (t < lead) p[t] = as_u(cast_to_float0((int32_t)p[t], it.scale));
    const int n4 = (len - lead) >> 2;
    u32x4* q = reinterpret_cast<u32x4*>(p + lead);
    for (int g = t; g < n4; g += 256) {
        u32x4 v = q[g];
#pragma unroll
        for (int i = 0; i < 4; i++) v[i] = as_u(cast_to_float0((int32_t)v[i], it.scale));
        q[g] = v;
    }
    const int done = lead + (n4 << 2);
    if (t < len - done) p[done + t] = as_u(cast_to_float0((int32_t)p[done + t], it.scale));
}

}  // namespace

void launch_canvas_cast(const CastArgs& a, hipStream_t s) {
    if (a.n <= 0 || a.first_block[a.n] <= 0) return;
    hipLaunchKernelGGL(k_canvas_cast, dim3((unsigned)a.first_block[a.n]), dim3(256), 0, s, a);
}

void launch_canvas_blend(const CanvasArgs& a, hipStream_t s) {
    if (a.n <= 0 || a.h <= 0 || a.w <= 0) return;
    int64_t grid = ((int64_t)(((a.w + 3) >> 2) + 1) * a.h + 255) / 256;
    if (grid > 16384) grid = 16384;
    hipLaunchKernelGGL(k_canvas_blend, dim3((unsigned)grid), dim3(256), 0, s, a);
}

}  // namespace jxl
