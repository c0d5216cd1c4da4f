// The per-sample arithmetic of JXLCodestreamDecoder's blend functions (JXLCodestreamDecoder.java:285-413), shared by k_blend
// (k_post.hip: one rectangle of one channel per launch) and k_patches (k_patch.hip: every patch position of a frame in one
// launch). "frame" and "ref" are the arguments blendMult / blendBlend / blendMulAdd receive under these names. One float operation
// per reference operation, in its order (the library is built with -ffp-contract=off; the division is the correctly rounded one).
#pragma once

namespace jxl {

// MathHelper.clampAsc(v, lo, hi) (a NaN passes through)
__device__ __forceinline__ float blend_clamp01(float v) { return v < 0.0f ? 0.0f : v > 1.0f ? 1.0f : v; }

// blendMult (:320-339)
__device__ __forceinline__ float blend_mult(float frame_s, float ref_s, bool clamp) {
    float nw = frame_s;
    if (clamp) nw = blend_clamp01(nw);
    return nw * ref_s;
}

// blendBlend with extra channels (:350-378). ref_alpha / frame_alpha are read by the caller only when !is_alpha
__device__ __forceinline__ float blend_blend(float frame_s, float ref_s, float frame_alpha, float ref_alpha, bool is_alpha, bool premult,
                                             bool clamp) {
    const float oldS = ref_s;
    const float newS = frame_s;
    const float oldA = is_alpha ? oldS : ref_alpha;
    float newA = is_alpha ? newS : frame_alpha;
    if (clamp) newA = blend_clamp01(newA);
    if (is_alpha) return oldA + newA * (1.0f - oldA);
    if (premult) return newS + oldS * (1.0f - newA);
    return (newS * newA + oldS * oldA * (1.0f - newA)) / (oldA + newA * (1.0f - oldA));
}

// blendMulAdd of a channel that is not the alpha channel, with extra channels (:393-411)
__device__ __forceinline__ float blend_muladd(float frame_s, float ref_s, float frame_alpha, bool clamp) {
    const float oldS = ref_s;
    const float newS = frame_s;
    float newA = frame_alpha;
    if (clamp) newA = blend_clamp01(newA);
    return oldS + newA * newS;
}

}  // namespace jxl
