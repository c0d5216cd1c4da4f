// JXLCodestreamDecoder.computePatches (JXLCodestreamDecoder.java:212-254) as a pixel-owned gather: every position of a frame in
// one launch. One workgroup = one non-empty 32 x 8 tile of the host's binning (patch_compile.h), one lane = one pixel, one wave =
// two rows of 32 (rows of 128 bytes), as in k_splines. The reference blends in place, in the order (patch, position, channel):
// a later application reads what an earlier one stored, a colour channel reads the frame's alpha plane that an alpha-channel
// application may have rewritten, and float sums do not commute with rounding -- but every read of one application is at the
// pixel it writes (frame side) or in a reference plane nothing writes. So the lane that owns a pixel walks its tile's list IN
// STAGE ORDER and, for each position whose rectangle holds the pixel and each channel in order, evaluates the reference's
// per-sample expression (jxl_blend.h) on what memory holds NOW and stores it: its own earlier stores come back through memory
// in program order, which also leaves the number of extra channels uncapped. No atomics, the same bits on every run; a pixel no
// position covers is never written.
// List indices, position records, op rows and the plane table are wave-uniform (they depend on blockIdx and loop counters only;
// the tables are const __restrict__): scalar loads. A position whose rows miss the wave's two rows is skipped by a scalar branch;
// only the rectangle test diverges.
#include "jxl_internal.h"
#include "jxl_blend.h"

namespace jxl {

__global__ __launch_bounds__(256) void k_patches(const int64_t* __restrict__ planes, int n_chan, int w, const PatchRec* __restrict__ rec,
                                                 const PatchOp* __restrict__ ops, const int32_t* __restrict__ tile,
                                                 const int32_t* __restrict__ start, const int32_t* __restrict__ list, int tiles_x) {
    const int t = tile[blockIdx.x];
    const int ty = t / tiles_x, tx = t - ty * tiles_x;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    const int wy0 = ty * kPatchTileH + wave * 2;  // the wave's two rows: wy0, wy0 + 1
    const int x = tx * kPatchTileW + (lane & 31), y = wy0 + (lane >> 5);
    const int64_t at = (int64_t)y * w + x;
    const int end = start[blockIdx.x + 1];
    for (int i = start[blockIdx.x]; i < end; i++) {
        const PatchRec p = rec[list[i]];
        if (p.y1 <= wy0 || p.y0 > wy0 + 1) continue;                  // wave-uniform
        if (x < p.x0 || x >= p.x1 || y < p.y0 || y >= p.y1) continue;  // (the rectangles lie inside the frame: such a pixel does too)
        const int64_t* slot = planes + (int64_t)n_chan * (1 + p.slot);
        const int rw = (int)planes[(int64_t)n_chan * 5 + p.slot];
        const int64_t rat = (int64_t)(y + p.dy) * rw + (x + p.dx);  // the pixel's sample in the slot's planes
        for (int d = 0; d < n_chan; d++) {
            const PatchOp o = ops[p.ops + d];
            if (o.op == POP_NONE) continue;
            uint32_t* F = reinterpret_cast<uint32_t*>(planes[d]);
            const uint32_t* R = reinterpret_cast<const uint32_t*>(slot[d]);
            if (o.op == POP_COPY_REF) {  // blendMulAdd on the alpha channel: copyToCanvas(ref) at frameOffset (:388-391)
                F[at] = R ? R[(int64_t)y * rw + x] : 0u;
                continue;
            }
            const uint32_t fs = F[at], rs = R ? R[rat] : 0u;  // (a NULL plane reads as zeros, int or float)
            if (o.op == POP_ADD_I) {  // blendAdd, int (:287-301)
                F[at] = rs + fs;
                continue;
            }
            // `frame` and `ref` as the blend function receives them: old = the frame plane, new = the slot's plane, swapped
            // for a below mode (:487-492)
            const bool below = (o.flags & kPatchBelow) != 0;
            const float frame_s = __uint_as_float(below ? rs : fs), ref_s = __uint_as_float(below ? fs : rs);
            const bool is_alpha = (o.flags & kPatchIsAlpha) != 0, clamp = (o.flags & kPatchClamp) != 0;
            float v;
            if (o.op == POP_ADD_F) {  // blendAdd, float (:303-316)
                v = ref_s + frame_s;
            } else if (o.op == POP_MULT) {
                v = blend_mult(frame_s, ref_s, clamp);
            } else {
                // frameAlpha is the FRAME's alpha plane at this pixel (:445), refAlpha the slot's (:444)
                float fa = 0.0f, ra = 0.0f;
                if (!is_alpha) {
                    fa = reinterpret_cast<const float*>(planes[o.alpha])[at];
                    if (o.op == POP_BLEND) {
                        const float* RA = reinterpret_cast<const float*>(slot[o.alpha]);
                        ra = RA ? RA[rat] : 0.0f;
                    }
                }
                v = o.op == POP_BLEND ? blend_blend(frame_s, ref_s, fa, ra, is_alpha, (o.flags & kPatchPremult) != 0, clamp)
                                      : blend_muladd(frame_s, ref_s, fa, clamp);
            }
            F[at] = __float_as_uint(v);
        }
    }
}

void launch_patches(const int64_t* planes, int n_chan, int w, const PatchRec* rec, const PatchOp* ops, const int32_t* tile,
                    const int32_t* start, const int32_t* list, int n_tiles, int tiles_x, hipStream_t s) {
    if (n_tiles <= 0) return;
    hipLaunchKernelGGL(k_patches, dim3((unsigned)n_tiles), dim3(256), 0, s, planes, n_chan, w, rec, ops, tile, start, list, tiles_x);
}

}  // namespace jxl
