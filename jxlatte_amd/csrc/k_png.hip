// The PNG's samples straight from the colour planes: stages 1-6 of k_color_convert (k_color.hip) and then k_pack's rule
// (k_post.hip; PNGWriter.java:79-111, 191-203) in one pass, without the three float planes the two kernels hand each other.
//
//   k_png_samples<NCH, BYTES>, per pixel:
//     1-6. cast, toLinearF, grey -> RGB, matrix, scale, fromLinearF       color_samples.h, in k_color_convert's order
//     7.   alpha: an int32 plane is cast with its tagged depth when PNGWriter coerces (premultiplied, or a depth other than
//          the PNG's), else it is clamped as it is; a float plane is taken as it is
//     8.   un-premultiply: colour / alpha, the correctly rounded float division
//     9.   (int)(v * max + 0.5f), clamped to 0..max                        ImageBuffer.castToInt0
//    10.   colour then alpha, 1 or 2 bytes a sample, big-endian option     writeIDAT's sample order
//   The float operations are those of the two-kernel path, in its order (file compiled with -ffp-contract=off): the bytes are
//   equal to jxl_stage_color_convert (float out) + jxl_stage_pack. The threshold-table quantisers of k_color_convert's integer
//   output are NOT used: they answer a different question (the reference's castToInt0 of the curve at 8 / 16 bits after a
//   round to nearest of the exact curve), and PNGWriter quantises the float.
//
// Shape: one lane owns 4 consecutive pixels: a 16-byte load per plane, and 4 * NCH * BYTES bytes of samples that leave in one
// store (12 bytes RGB8, 16 bytes RGBA8 / grey+alpha 16) or two (24 bytes RGB16, 32 bytes RGBA16) instead of one byte or short
// per lane-instruction. The 4 pixels go through ONE copy of the stage code: a rolled loop that takes its inputs from the front
// of the loaded vectors (rotated by one element per round) and pushes the pixel's bits in at the top of a shift register of
// 4 * NCH * BYTES bytes, which moves down by one pixel per round -- constant shift counts, no indexed registers, and the f64
// chains of the curves exist once per channel, as in k_color_convert (one fp_pow live at a time).
// The last group of a plane whose size is no multiple of 4 loads and stores sample by sample (one lane of the grid).
#include "color_samples.h"

namespace jxl {
namespace {

template <int NCH, int BYTES>
struct PngShape {
    static constexpr int kColors = NCH <= 2 ? 1 : 3;
    static constexpr bool kAlpha = (NCH & 1) == 0;
    static constexpr int kPixelBits = NCH * BYTES * 8;               // 8 .. 64
    static constexpr int kPixelWords = (kPixelBits + 31) / 32;       // 1 or 2
    static constexpr int kWords = 4 * NCH * BYTES / 4;               // the lane's 4 pixels: 1 .. 8 words
};

// one pixel: the words of its colour planes (w[c], c < n_planes) and of its alpha plane -> NCH samples, each below 2^(8 BYTES)
template <int NCH, int BYTES>
__device__ __forceinline__ void png_pixel(const PngArgs& p, const uint32_t w[3], uint32_t aw, uint32_t q[4]) {
    using S = PngShape<NCH, BYTES>;
    const int maxv = BYTES == 1 ? 255 : 65535;
    float v[3];
    color_stages<S::kColors>(p.c, w, v);
    if (S::kAlpha) {
        float fa = __builtin_bit_cast(float, aw);
        if (p.alpha_is_int) fa = (float)(int32_t)aw * p.alpha_scale;  // castToFloat0 with the tagged depth
        if (p.premultiplied) {
#pragma unroll
            for (int c = 0; c < S::kColors; c++) v[c] = v[c] / fa;
        }
        if (p.alpha_is_int && !p.alpha_coerce) {
            const int32_t ia = (int32_t)aw;
            q[S::kColors] = (uint32_t)(ia < 0 ? 0 : ia > maxv ? maxv : ia);
        } else {
            q[S::kColors] = (uint32_t)cast_to_int0(fa, maxv);
        }
    }
#pragma unroll
    for (int c = 0; c < S::kColors; c++) q[c] = (uint32_t)cast_to_int0(v[c], maxv);
}

template <int NCH, int BYTES>
__global__ __launch_bounds__(256) void k_png_samples(const PngArgs p) {
    using S = PngShape<NCH, BYTES>;
    constexpr int W = S::kWords, PW = S::kPixelWords, B = S::kPixelBits;
    const ColorArgs& a = p.c;
    const int64_t groups = (a.n + 3) >> 2;
    for (int64_t g = blockIdx.x * 256LL + threadIdx.x; g < groups; g += (int64_t)gridDim.x * 256) {
        const int64_t i0 = g << 2;
        const bool full = i0 + 4 <= a.n;
        uint4 in[3] = {make_uint4(0, 0, 0, 0), make_uint4(0, 0, 0, 0), make_uint4(0, 0, 0, 0)}, al = make_uint4(0, 0, 0, 0);
        if (full) {
#pragma unroll
            for (int c = 0; c < 3; c++)
                if (c < a.n_planes) in[c] = *reinterpret_cast<const uint4*>((const uint32_t*)a.in[c] + i0);
            if (S::kAlpha) al = *reinterpret_cast<const uint4*>((const uint32_t*)p.alpha + i0);
        } else {
            const int cnt = (int)(a.n - i0);  // 1..3
#pragma unroll
            for (int c = 0; c < 3; c++) {
                if (c >= a.n_planes) continue;
                const uint32_t* s = (const uint32_t*)a.in[c] + i0;
                in[c] = make_uint4(s[0], cnt > 1 ? s[1] : 0u, cnt > 2 ? s[2] : 0u, 0u);
            }
            if (S::kAlpha) {
                const uint32_t* s = (const uint32_t*)p.alpha + i0;
                al = make_uint4(s[0], cnt > 1 ? s[1] : 0u, cnt > 2 ? s[2] : 0u, 0u);
            }
        }
        uint32_t reg[W + PW];  // [0, W): the samples of the pixels done so far, the latest on top; [W, W + PW): the new pixel
#pragma unroll
        for (int j = 0; j < W + PW; j++) reg[j] = 0;
#pragma unroll 1
        for (int k = 0; k < 4; k++) {
            const uint32_t w[3] = {in[0].x, in[1].x, in[2].x};
            uint32_t q[4] = {0, 0, 0, 0};
            png_pixel<NCH, BYTES>(p, w, al.x, q);
#pragma unroll
            for (int c = 0; c < 3; c++) in[c] = make_uint4(in[c].y, in[c].z, in[c].w, in[c].x);
            al = make_uint4(al.y, al.z, al.w, al.x);
            if (BYTES == 1) {
                reg[W] = q[0] | (q[1] << 8) | (q[2] << 16) | (q[3] << 24);
            } else {
                if (p.big_endian) {
#pragma unroll
                    for (int c = 0; c < 4; c++) q[c] = ((q[c] & 0xffu) << 8) | (q[c] >> 8);
                }
                reg[W] = q[0] | (q[1] << 16);
                if (PW == 2) reg[W + PW - 1] = q[2] | (q[3] << 16);
            }
            // down by one pixel; the new pixel comes in at the top
#pragma unroll
            for (int j = 0; j < W; j++) {
                constexpr int ws = B / 32, bs = B % 32;
                if constexpr (bs == 0) reg[j] = reg[j + ws];
                else reg[j] = (reg[j + ws] >> bs) | (reg[j + ws + 1] << (32 - bs));
            }
        }
        uint32_t* o = (uint32_t*)p.out + g * W;
        // The 12- and 24-byte shapes have no vector type of their own alignment: they are written as adjacent dword / 8-byte stores
        // that hipcc's load-store vectoriser joins (gfx950: global_store_dwordx3; dwordx4 + dwordx2). That is the optimiser's doing:
        // after a compiler change, count the global_store_* of the eight instances again (DESIGN 4.5e has the expected counts).
        if (full) {
            if (W == 4) {
                *reinterpret_cast<uint4*>(o) = make_uint4(reg[0], reg[1], reg[2], reg[3]);
            } else if (W == 8) {
                *reinterpret_cast<uint4*>(o) = make_uint4(reg[0], reg[1], reg[2], reg[3]);
                *reinterpret_cast<uint4*>(o + 4) = make_uint4(reg[4], reg[5], reg[6], reg[7]);
            } else if (W == 2 || W == 6) {  // 8 or 24 bytes, 8-byte aligned
#pragma unroll
                for (int j = 0; j < W; j += 2) *reinterpret_cast<uint2*>(o + j) = make_uint2(reg[j], reg[j + 1]);
            } else {  // 4 or 12 bytes
#pragma unroll
                for (int j = 0; j < W; j++) o[j] = reg[j];
            }
        } else {
            const int nbytes = (int)(a.n - i0) * NCH * BYTES;
            uint8_t* ob = (uint8_t*)o;
#pragma unroll
            for (int b = 0; b < 3 * NCH * BYTES; b++)
                if (b < nbytes) ob[b] = (uint8_t)(reg[b >> 2] >> (8 * (b & 3)));
        }
    }
}

template <int NCH, int BYTES>
void launch_png(const PngArgs& p, hipStream_t s) {
    int64_t grid = ((p.c.n + 3) / 4 + 255) / 256;
    if (grid > 8192) grid = 8192;
    hipLaunchKernelGGL((k_png_samples<NCH, BYTES>), dim3((unsigned)grid), dim3(256), 0, s, p);
}

}  // namespace

void launch_png_samples(const PngArgs& p, int n_color, hipStream_t s) {
    if (p.c.n <= 0) return;
    const int nch = n_color + (p.alpha ? 1 : 0);
    const bool wide = p.bit_depth == 16;
    switch (nch) {
        case 1: wide ? launch_png<1, 2>(p, s) : launch_png<1, 1>(p, s); break;
        case 2: wide ? launch_png<2, 2>(p, s) : launch_png<2, 1>(p, s); break;
        case 3: wide ? launch_png<3, 2>(p, s) : launch_png<3, 1>(p, s); break;
        default: wide ? launch_png<4, 2>(p, s) : launch_png<4, 1>(p, s); break;
    }
}

}  // namespace jxl
