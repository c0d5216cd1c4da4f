// The PFM's samples straight from the image's planes (PFMWriter.java:22-49 with ImageBuffer.castToFloat): no colour stage at
// all -- the file holds the image's own samples.
//
//   k_pfm_samples<NCH, IN_INT>, per sample:
//     1. cast: an int32 plane gives (float)v * scale[c], scale[c] = 1.0f / max of its tagged depth, the IEEE quotient made on
//        the host (ImageBuffer.java:115-119: the conversion rounds first, then ONE f32 multiply); a float plane is taken as it is
//     2. Float.floatToIntBits: every NaN becomes 0x7fc00000; -0.0f, the infinities and the subnormals keep their bits
//     3. DataOutputStream.writeFloat: the four bytes, most significant first
//     4. channels interleaved per pixel, pixels left to right, rows BOTTOM TO TOP: input row y is output row H - 1 - y
//   Which plane is int32 is a kernel argument per plane (is_int[c]): planes of mixed kind are legal in the reference. IN_INT says
//   only whether ANY plane is: the all-float instances (the resident planes' case) hold no conversion code. The float steps are
//   one conversion and one multiply (file compiled with -ffp-contract=off like every other; there is nothing to contract).
//
// Shape (k_png.hip's): one lane owns 4 consecutive pixels of a row: a 16-byte load per plane, and 16 * NCH bytes of samples that
// leave as one (grey) or three (RGB: 48 contiguous bytes) 16-byte stores. Rows are W floats in and NCH * W words out, neither
// padded: unless W is a multiple of 4 the lane's addresses are only 4-byte aligned, so the vectors are declared with that
// alignment (u32x4a) and the compiler is told the truth; gfx950 code objects run with unaligned access enabled and hipcc keeps
// them as global_load_dwordx4 / global_store_dwordx4 (DESIGN 4.5f has the counts to look for after a compiler change).
// The last group of a row whose width is no multiple of 4 loads and stores sample by sample.
#include "jxl_internal.h"

namespace jxl {
namespace {

typedef uint32_t u32x4a __attribute__((ext_vector_type(4), aligned(4)));

__device__ __forceinline__ uint32_t pfm_word(uint32_t w, bool is_int, float scale) {
    if (is_int) w = __builtin_bit_cast(uint32_t, (float)(int32_t)w * scale);
    if ((w & 0x7fffffffu) > 0x7f800000u) w = 0x7fc00000u;  // floatToIntBits
    return __builtin_bswap32(w);
}

template <int NCH, bool IN_INT>
__global__ __launch_bounds__(256) void k_pfm_samples(const PfmArgs p) {
    const int64_t gpr = ((int64_t)p.w + 3) >> 2;  // groups per row
    const int64_t groups = gpr * p.h;
    for (int64_t g = blockIdx.x * 256LL + threadIdx.x; g < groups; g += (int64_t)gridDim.x * 256) {
        const int64_t y = g / gpr;
        const int x0 = (int)(g - y * gpr) << 2;
        const int cnt = p.w - x0;  // >= 1
        const int64_t i0 = y * p.w + x0;
        uint32_t* o = (uint32_t*)p.out + ((int64_t)(p.h - 1 - y) * p.w + x0) * NCH;
        if (cnt >= 4) {
            u32x4a v[NCH];
#pragma unroll
            for (int c = 0; c < NCH; c++) {
                v[c] = *reinterpret_cast<const u32x4a*>((const uint32_t*)p.in[c] + i0);
#pragma unroll
                for (int k = 0; k < 4; k++) v[c][k] = pfm_word(v[c][k], IN_INT && p.is_int[c], p.scale[c]);
            }
            if constexpr (NCH == 1) {
                *reinterpret_cast<u32x4a*>(o) = v[0];
            } else {
                u32x4a s0, s1, s2;
                s0[0] = v[0][0]; s0[1] = v[1][0]; s0[2] = v[2][0]; s0[3] = v[0][1];
                s1[0] = v[1][1]; s1[1] = v[2][1]; s1[2] = v[0][2]; s1[3] = v[1][2];
                s2[0] = v[2][2]; s2[1] = v[0][3]; s2[2] = v[1][3]; s2[3] = v[2][3];
                *reinterpret_cast<u32x4a*>(o) = s0;
                *reinterpret_cast<u32x4a*>(o + 4) = s1;
                *reinterpret_cast<u32x4a*>(o + 8) = s2;
            }
        } else {
            for (int k = 0; k < cnt; k++) {
#pragma unroll
                for (int c = 0; c < NCH; c++)
                    o[k * NCH + c] = pfm_word(((const uint32_t*)p.in[c])[i0 + k], IN_INT && p.is_int[c], p.scale[c]);
            }
        }
    }
}

template <int NCH, bool IN_INT>
void launch_pfm(const PfmArgs& p, hipStream_t s) {
    int64_t grid = ((((int64_t)p.w + 3) / 4) * p.h + 255) / 256;
    if (grid > 16384) grid = 16384;
    hipLaunchKernelGGL((k_pfm_samples<NCH, IN_INT>), dim3((unsigned)grid), dim3(256), 0, s, p);
}

}  // namespace

void launch_pfm_samples(const PfmArgs& p, hipStream_t s) {
    if (p.h <= 0 || p.w <= 0) return;
    bool any_int = false;
    for (int c = 0; c < p.n_planes; c++) any_int = any_int || p.is_int[c];
    if (p.n_planes == 1) any_int ? launch_pfm<1, true>(p, s) : launch_pfm<1, false>(p, s);
    else any_int ? launch_pfm<3, true>(p, s) : launch_pfm<3, false>(p, s);
}

}  // namespace jxl
