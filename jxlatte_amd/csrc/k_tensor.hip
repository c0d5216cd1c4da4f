// The image as a device tensor straight from its planes: stages 1-6 of k_color_convert and k_png_samples' alpha rule, then what a
// tensor consumer wants instead of the PNG's bytes -- in one pass, into memory the caller owns.
//
//   k_tensor_samples<BYTES, NCH, LAYOUT>, per pixel:
//     1-6. cast, toLinearF, grey -> RGB, matrix, scale, fromLinearF       color_samples.h: color_stages, as k_png_samples
//     7.   alpha: a float plane as it is; an int32 plane cast with its tagged depth
//     8.   un-premultiply: colour / alpha, the correctly rounded float division (whether or not alpha is written)
//     9.   float dtypes: (v - mean[c]) * inv_std[c], two roundings, c the output channel
//    10.   F32 the bits; F16 / BF16 round to nearest even, every NaN the canonical quiet one; U8 castToInt0(v, 255), and for an
//          int32 alpha plane png_pixel's rule at 8 bits (clamped as it is unless PNGWriter would coerce it)
//    11.   CHW: channel c at out + c * n elements; HWC: the channels of a pixel side by side
//   The float operations are those of jxl_stage_color_convert in its order (file compiled with -ffp-contract=off).
//
// Shape (k_png.hip's): one lane owns 4 consecutive pixels, a 16-byte load per input plane, and a rolled 4-round loop through ONE
// copy of the stage code (the f64 chains of the curves exist once per channel). HWC keeps k_png's shift register of the lane's
// 4 * NCH * BYTES bytes; CHW keeps one of 4 * BYTES bytes per channel. A full group leaves in stores of up to 16 bytes when the
// launch is `wide`: the host has checked that every group's address has the alignment its widest store needs
// (tensor_check.h: tensor_wide_ok -- `out` is only element-aligned, and the planes 1.. of a CHW tensor of odd size are not even
// that of a dword for the 1- and 2-byte dtypes). Otherwise, and in the last group of a size that is no multiple of 4, the samples
// leave one by one. BF16 and F16 share the 2-byte instances (a wave-uniform branch at the conversion).
#include "color_samples.h"
#include "tensor_store.h"

namespace jxl {
namespace {

template <int BYTES, int NCH>
struct TensorShape {
    static constexpr int kColors = NCH <= 2 ? 1 : 3;
    static constexpr bool kAlphaOut = (NCH & 1) == 0;
    static constexpr int kPixelBits = NCH * BYTES * 8;          // 8 .. 128
    static constexpr int kPixelWords = (kPixelBits + 31) / 32;  // 1 .. 4
    static constexpr int kWords = NCH * BYTES;                  // the lane's 4 pixels: 1 .. 16 words
};

// one pixel: the words of its colour planes and of its alpha plane -> the bits of its NCH elements
template <int BYTES, int NCH>
__device__ __forceinline__ void tensor_pixel(const TensorArgs& t, const uint32_t w[3], uint32_t aw, uint32_t q[4]) {
    using S = TensorShape<BYTES, NCH>;
    const PngArgs& p = t.g;
    float v[3];
    color_stages<S::kColors>(p.c, w, v);
    float fa = 0.0f;
    if (p.alpha) {  // (wave-uniform: set only where alpha is written or divides)
        fa = __builtin_bit_cast(float, aw);
        if (p.alpha_is_int) fa = (float)(int32_t)aw * p.alpha_scale;  // castToFloat0 with the tagged depth
        if (p.premultiplied) {
#pragma unroll
            for (int c = 0; c < S::kColors; c++) v[c] = v[c] / fa;
        }
    }
    if (BYTES == 1) {
#pragma unroll
        for (int c = 0; c < S::kColors; c++) q[c] = (uint32_t)cast_to_int0(v[c], 255);
        if (S::kAlphaOut) {
            if (p.alpha_is_int && !p.alpha_coerce) {
                const int32_t ia = (int32_t)aw;
                q[S::kColors] = (uint32_t)(ia < 0 ? 0 : ia > 255 ? 255 : ia);
            } else {
                q[S::kColors] = (uint32_t)cast_to_int0(fa, 255);
            }
        }
    } else {
        float o[4] = {v[0], S::kColors == 3 ? v[1] : fa, S::kColors == 3 ? v[2] : 0.0f, fa};
        if (t.use_norm) {
#pragma unroll
            for (int c = 0; c < NCH; c++) o[c] = (o[c] - t.mean[c]) * t.inv_std[c];
        }
#pragma unroll
        for (int c = 0; c < NCH; c++) q[c] = tensor_float_bits<BYTES>(o[c], t.dtype);
    }
}

template <int BYTES, int NCH, int LAYOUT>
__global__ __launch_bounds__(256) void k_tensor_samples(const TensorArgs t) {
    using S = TensorShape<BYTES, NCH>;
    const PngArgs& p = t.g;
    const ColorArgs& a = p.c;
    const int64_t n = a.n;
    const int64_t groups = (n + 3) >> 2;
    for (int64_t g = blockIdx.x * 256LL + threadIdx.x; g < groups; g += (int64_t)gridDim.x * 256) {
        const int64_t i0 = g << 2;
        const bool full = i0 + 4 <= n;
        const int cnt = full ? 4 : (int)(n - i0);  // 1..4
        uint4 in[3] = {make_uint4(0, 0, 0, 0), make_uint4(0, 0, 0, 0), make_uint4(0, 0, 0, 0)}, al = make_uint4(0, 0, 0, 0);
        if (full) {
#pragma unroll
            for (int c = 0; c < 3; c++)
                if (c < a.n_planes) in[c] = *reinterpret_cast<const uint4*>((const uint32_t*)a.in[c] + i0);
            if (p.alpha) al = *reinterpret_cast<const uint4*>((const uint32_t*)p.alpha + i0);
        } else {
#pragma unroll
            for (int c = 0; c < 3; c++) {
                if (c >= a.n_planes) continue;
                const uint32_t* s = (const uint32_t*)a.in[c] + i0;
                in[c] = make_uint4(s[0], cnt > 1 ? s[1] : 0u, cnt > 2 ? s[2] : 0u, 0u);
            }
            if (p.alpha) {
                const uint32_t* s = (const uint32_t*)p.alpha + i0;
                al = make_uint4(s[0], cnt > 1 ? s[1] : 0u, cnt > 2 ? s[2] : 0u, 0u);
            }
        }
        if (LAYOUT == JXL_TENSOR_HWC) {
            constexpr int W = S::kWords, PW = S::kPixelWords, B = S::kPixelBits;
            uint32_t reg[W + PW];  // [0, W): the pixels done so far, the latest on top; [W, W + PW): the new pixel
#pragma unroll
            for (int j = 0; j < W + PW; j++) reg[j] = 0;
#pragma unroll 1
            for (int k = 0; k < 4; k++) {
                const uint32_t w[3] = {in[0].x, in[1].x, in[2].x};
                uint32_t q[4] = {0, 0, 0, 0};
                tensor_pixel<BYTES, NCH>(t, w, al.x, q);
#pragma unroll
                for (int c = 0; c < 3; c++) in[c] = make_uint4(in[c].y, in[c].z, in[c].w, in[c].x);
                al = make_uint4(al.y, al.z, al.w, al.x);
                if (BYTES == 1) {
                    reg[W] = q[0] | (q[1] << 8) | (q[2] << 16) | (q[3] << 24);
                } else if (BYTES == 2) {
                    reg[W] = q[0] | (q[1] << 16);
                    if (PW == 2) reg[W + PW - 1] = q[2] | (q[3] << 16);
                } else {
#pragma unroll
                    for (int c = 0; c < NCH; c++) reg[W + c] = q[c];
                }
#pragma unroll
                for (int j = 0; j < W; j++) {  // down by one pixel; the new pixel comes in at the top
                    constexpr int ws = B / 32, bs = B % 32;
                    if constexpr (bs == 0) reg[j] = reg[j + ws];
                    else reg[j] = (reg[j + ws] >> bs) | (reg[j + ws + 1] << (32 - bs));
                }
            }
            if (full && t.wide) {
                store_words<W>((uint32_t*)((uint8_t*)t.out + g * (4 * NCH * BYTES)), reg);
            } else {
#pragma unroll
                for (int e = 0; e < 4 * NCH; e++)
                    if (e < cnt * NCH) store_element<BYTES>(t.out, i0 * NCH + e, reg, e);
            }
        } else {
            constexpr int W = BYTES;  // words of one channel's 4 elements
            uint32_t reg[NCH][W + 1];  // per channel: [0, W) the elements done so far, the latest on top; [W]: the new element
#pragma unroll
            for (int c = 0; c < NCH; c++)
#pragma unroll
                for (int j = 0; j <= W; j++) reg[c][j] = 0;
#pragma unroll 1
            for (int k = 0; k < 4; k++) {
                const uint32_t w[3] = {in[0].x, in[1].x, in[2].x};
                uint32_t q[4] = {0, 0, 0, 0};
                tensor_pixel<BYTES, NCH>(t, w, al.x, q);
#pragma unroll
                for (int c = 0; c < 3; c++) in[c] = make_uint4(in[c].y, in[c].z, in[c].w, in[c].x);
                al = make_uint4(al.y, al.z, al.w, al.x);
#pragma unroll
                for (int c = 0; c < NCH; c++) {
                    reg[c][W] = q[c];
#pragma unroll
                    for (int j = 0; j < W; j++) {  // down by one element
                        constexpr int bs = (BYTES * 8) % 32;
                        if constexpr (bs == 0) reg[c][j] = reg[c][j + 1];
                        else reg[c][j] = (reg[c][j] >> bs) | (reg[c][j + 1] << (32 - bs));
                    }
                }
            }
#pragma unroll
            for (int c = 0; c < NCH; c++) {
                const int64_t at = (int64_t)c * n + i0;  // element index of the group in channel c
                if (full && t.wide) {
                    store_words<W>((uint32_t*)((uint8_t*)t.out + at * BYTES), reg[c]);
                } else {
#pragma unroll
                    for (int e = 0; e < 4; e++)
                        if (e < cnt) store_element<BYTES>(t.out, at + e, reg[c], e);
                }
            }
        }
    }
}

template <int BYTES, int NCH>
void launch_tensor(const TensorArgs& t, hipStream_t s, int max_workgroups) {
    int64_t grid = ((t.g.c.n + 3) / 4 + 255) / 256;
    if (grid > 8192) grid = 8192;
    if (max_workgroups > 0 && grid > max_workgroups) grid = max_workgroups;
    if (t.layout == JXL_TENSOR_HWC)
        hipLaunchKernelGGL((k_tensor_samples<BYTES, NCH, JXL_TENSOR_HWC>), dim3((unsigned)grid), dim3(256), 0, s, t);
    else
        hipLaunchKernelGGL((k_tensor_samples<BYTES, NCH, JXL_TENSOR_CHW>), dim3((unsigned)grid), dim3(256), 0, s, t);
}

template <int BYTES>
void launch_tensor_nch(const TensorArgs& t, hipStream_t s, int max_workgroups) {
    switch (t.n_out) {
        case 1: launch_tensor<BYTES, 1>(t, s, max_workgroups); break;
        case 2: launch_tensor<BYTES, 2>(t, s, max_workgroups); break;
        case 3: launch_tensor<BYTES, 3>(t, s, max_workgroups); break;
        default: launch_tensor<BYTES, 4>(t, s, max_workgroups); break;
    }
}

}  // namespace

void launch_tensor_samples(const TensorArgs& t, hipStream_t s, int max_workgroups) {
    if (t.g.c.n <= 0) return;
    if (t.dtype == JXL_TENSOR_U8) launch_tensor_nch<1>(t, s, max_workgroups);
    else if (t.dtype == JXL_TENSOR_F32) launch_tensor_nch<4>(t, s, max_workgroups);
    else launch_tensor_nch<2>(t, s, max_workgroups);
}

}  // namespace jxl
