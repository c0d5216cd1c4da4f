// One output tile of the resized tensor exit: the body both k_tensor_resize (one image per launch) and k_tensor_resize_batch
// (a work list over N images) run, so that the arithmetic exists once -- the way color_stages became color_front + color_back.
//
//   resize_tile<BYTES, COLORS>(r, tile, lds), called by all 256 lanes of a workgroup with wave-uniform r and tile:
//   V pass  a lane owns 4 consecutive source columns of the tile's footprint (its start aligned down to 4; a footprint wider
//           than 1024 columns in chunks) and walks the footprint's rows top to bottom: one 16-byte load per plane and row
//           (wide_in; else dwords), stages 1-5 of color_samples.h in registers (color_front; alpha: a float plane as it is, an
//           int32 plane cast with its tagged depth), and for each tile row t whose tap range holds the row
//             acc[t] = wy[0] * S  on the range's first row,  acc[t] = acc[t] + wy[k] * S  on the others.
//           Row ranges and weights are wave-uniform (scalar loads); a source row is loaded once per tile. No LDS, no cross-lane
//           step: the pass that touches every source pixel is loads and VALU only.
//   LDS     the vertical sums, th x planes lines of the footprint's width; column x sits at x + (x >> 5) (skew): at the 16-dword
//           lane stride of a 16:1 reduction a plain line would put every lane of a half-wave on one of two banks.
//   H pass  a lane owns one output pixel: R = wx[0] * V(first), R = R + wx[k] * V(first + k), every plane, then stage 6
//           (color_back), colour / alpha when premultiplied, the normalisation, the conversion and the store of k_tensor.hip's
//           tensor_pixel -- except that U8 alpha is cast_to_int0 of the FILTERED float alpha (there is no integer to clamp).
//   Every sum is one lane's, sequential in ascending index: no tile or grid choice changes a bit (-ffp-contract=off).
// The body ends behind a barrier: the next tile of the workgroup -- of this descriptor or of another, whose LDS image may be laid
// out differently -- writes the image again. Everything the body branches on but the lane's own columns and pixel comes from r
// and the tile index: it stays wave-uniform whatever descriptor the next tile brings.
// Bounds: the host's tables keep every tap range inside the box and the box inside the planes, first and first + count monotone
// (tensor_resize_check.h); the footprint of a tile is therefore what its first and last row and column say.
#ifndef JXL_TENSOR_RESIZE_BODY_H
#define JXL_TENSOR_RESIZE_BODY_H
#include "color_samples.h"
#include "tensor_store.h"

namespace jxl {

// the tiles of one descriptor
__host__ __device__ inline int64_t resize_tiles(const ResizeArgs& r) {
    return (int64_t)((r.ow + r.tw - 1) / r.tw) * ((r.oh + r.th - 1) / r.th);
}

template <int BYTES, int COLORS>
__device__ __forceinline__ void resize_tile(const ResizeArgs& r, const int64_t tile, float* lds) {
    constexpr int PL = COLORS + 1;  // register planes: the colours and alpha
    const TensorArgs& t = r.t;
    const PngArgs& p = t.g;
    const ColorArgs& a = p.c;
    const bool has_a = p.alpha != nullptr;  // (wave-uniform: the plane is read -- written or dividing)
    const int P = r.planes, lw = r.lds_w;
    const int skew = r.skew ? -1 : 0;
    const int tid = (int)threadIdx.x;
    const int tiles_x = (r.ow + r.tw - 1) / r.tw;
    const int ox0 = (int)(tile % tiles_x) * r.tw, oy0 = (int)(tile / tiles_x) * r.th;
    const int ox1 = ox0 + r.tw < r.ow ? ox0 + r.tw : r.ow, oy1 = oy0 + r.th < r.oh ? oy0 + r.th : r.oh;
    const int nrow = oy1 - oy0;
    // the footprint: columns [fx0, fx1) from ax0, rows [ry0, ry1)
    const int fx0 = r.x0 + r.xfirst[ox0];
    const int fx1 = r.x0 + r.xfirst[ox1 - 1] + (r.xoff[ox1] - r.xoff[ox1 - 1]);
    const int ax0 = fx0 & ~3;
    const int ry0 = r.y0 + r.yfirst[oy0];
    const int ry1 = r.y0 + r.yfirst[oy1 - 1] + (r.yoff[oy1] - r.yoff[oy1 - 1]);
    int rf[4], rn[4], ro[4];  // per tile row: first source row, rows, offset of its weights
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int oy = oy0 + (i < nrow ? i : 0);
        rf[i] = r.y0 + r.yfirst[oy];
        ro[i] = r.yoff[oy];
        rn[i] = i < nrow ? r.yoff[oy + 1] - ro[i] : 0;
    }

    for (int cb = 0; ax0 + cb < fx1; cb += 1024) {
        const int c4 = ax0 + cb + 4 * tid;  // the lane's 4 columns
        if (c4 < fx1) {
            float acc[4][PL][4];
#pragma unroll
            for (int i = 0; i < 4; i++)
#pragma unroll
                for (int c = 0; c < PL; c++)
#pragma unroll
                    for (int k = 0; k < 4; k++) acc[i][c][k] = 0.0f;
            // one row of the lane's 4 columns: the words of the colour planes and of the alpha plane
            auto load_row = [&](int y, uint4 in[3], uint4& al) {
                const int64_t at = (int64_t)y * r.src_w + c4;
                in[0] = in[1] = in[2] = al = make_uint4(0, 0, 0, 0);
                if (r.wide_in) {  // (c4 is a multiple of 4 below a width that is one: the 4 columns are the row's)
#pragma unroll
                    for (int c = 0; c < COLORS; c++)
                        if (c < a.n_planes) in[c] = *reinterpret_cast<const uint4*>((const uint32_t*)a.in[c] + at);
                    if (has_a) al = *reinterpret_cast<const uint4*>((const uint32_t*)p.alpha + at);
                } else {
                    const int cnt = fx1 - c4;  // >= 1 columns of the footprint from c4 on
#pragma unroll
                    for (int c = 0; c < COLORS; c++) {
                        if (c >= a.n_planes) continue;
                        const uint32_t* s = (const uint32_t*)a.in[c] + at;
                        in[c] = make_uint4(s[0], cnt > 1 ? s[1] : 0u, cnt > 2 ? s[2] : 0u, cnt > 3 ? s[3] : 0u);
                    }
                    if (has_a) {
                        const uint32_t* s = (const uint32_t*)p.alpha + at;
                        al = make_uint4(s[0], cnt > 1 ? s[1] : 0u, cnt > 2 ? s[2] : 0u, cnt > 3 ? s[3] : 0u);
                    }
                }
            };
            uint4 nin[3], nal;  // the next row, asked for before this one is worked on
            load_row(ry0, nin, nal);
            for (int y = ry0; y < ry1; y++) {
                uint4 in[3] = {nin[0], nin[1], nin[2]}, al = nal;
                if (y + 1 < ry1) load_row(y + 1, nin, nal);
                // stages 1-5 of the 4 pixels through ONE copy of the stage code (k_tensor.hip's rolled loop)
                float sv[PL][4];
#pragma unroll
                for (int c = 0; c < PL; c++)
#pragma unroll
                    for (int k = 0; k < 4; k++) sv[c][k] = 0.0f;
#pragma unroll 1
                for (int k = 0; k < 4; k++) {
                    const uint32_t w[3] = {in[0].x, in[1].x, in[2].x};
                    float v[3] = {0.0f, 0.0f, 0.0f};
                    color_front<COLORS>(a, w, v);
                    float fa = 0.0f;
                    if (has_a) {
                        fa = __builtin_bit_cast(float, al.x);
                        if (p.alpha_is_int) fa = (float)(int32_t)al.x * p.alpha_scale;  // castToFloat0 with the tagged depth
                    }
#pragma unroll
                    for (int c = 0; c < 3; c++) in[c] = make_uint4(in[c].y, in[c].z, in[c].w, in[c].x);
                    al = make_uint4(al.y, al.z, al.w, al.x);
#pragma unroll
                    for (int c = 0; c < PL; c++) {
                        sv[c][0] = sv[c][1], sv[c][1] = sv[c][2], sv[c][2] = sv[c][3];
                        sv[c][3] = c < COLORS ? v[c] : fa;
                    }
                }
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const int k = y - rf[i];
                    if (k < 0 || k >= rn[i]) continue;  // (wave-uniform)
                    const float wy = r.wy[ro[i] + k];
                    if (k == 0) {
#pragma unroll
                        for (int c = 0; c < PL; c++)
#pragma unroll
                            for (int j = 0; j < 4; j++) acc[i][c][j] = wy * sv[c][j];
                    } else {
#pragma unroll
                        for (int c = 0; c < PL; c++)
#pragma unroll
                            for (int j = 0; j < 4; j++) acc[i][c][j] = acc[i][c][j] + wy * sv[c][j];
                    }
                }
            }
            const int lx = c4 - ax0;
#pragma unroll
            for (int i = 0; i < 4; i++) {
                if (i >= nrow) continue;
#pragma unroll
                for (int c = 0; c < PL; c++) {
                    if (c >= P) continue;  // (alpha is the plane after the colours, when it is read)
                    float* line = lds + (i * P + c) * lw;
#pragma unroll
                    for (int j = 0; j < 4; j++) line[lx + j + (((lx + j) >> 5) & skew)] = acc[i][c][j];
                }
            }
        }
    }
    __syncthreads();

    const int tcol = tid % r.tw, trow = tid / r.tw;
    if (trow < nrow && ox0 + tcol < ox1) {
        const int ox = ox0 + tcol, oy = oy0 + trow;
        const int xf = r.x0 + r.xfirst[ox] - ax0;
        const int o0 = r.xoff[ox], n = r.xoff[ox + 1] - o0;
        const float* line = lds + trow * P * lw;
        float R[PL];
        {
            const float wx = r.wx[o0];
            const int lc = xf + ((xf >> 5) & skew);
#pragma unroll
            for (int c = 0; c < PL; c++) R[c] = c < P ? wx * line[c * lw + lc] : 0.0f;
        }
        for (int k = 1; k < n; k++) {
            const float wx = r.wx[o0 + k];
            const int x = xf + k, lc = x + ((x >> 5) & skew);
#pragma unroll
            for (int c = 0; c < PL; c++)
                if (c < P) R[c] = R[c] + wx * line[c * lw + lc];
        }
        // tensor_pixel behind stage 5
        float v[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int c = 0; c < COLORS; c++) v[c] = color_back(a, R[c]);
        const float fa = has_a ? R[COLORS] : 0.0f;
        if (has_a && p.premultiplied) {
#pragma unroll
            for (int c = 0; c < COLORS; c++) v[c] = v[c] / fa;
        }
        const int n_out = t.n_out;  // COLORS, + 1 when alpha is written
        uint32_t q[4] = {0, 0, 0, 0};
        if (BYTES == 1) {
#pragma unroll
            for (int c = 0; c < COLORS; c++) q[c] = (uint32_t)cast_to_int0(v[c], 255);
            q[COLORS] = (uint32_t)cast_to_int0(fa, 255);
        } else {
            float o[4] = {v[0], COLORS == 3 ? v[1] : fa, COLORS == 3 ? v[2] : 0.0f, fa};
            if (t.use_norm) {
#pragma unroll
                for (int c = 0; c < PL; c++) o[c] = (o[c] - t.mean[c]) * t.inv_std[c];
            }
#pragma unroll
            for (int c = 0; c < PL; c++) q[c] = tensor_float_bits<BYTES>(o[c], t.dtype);
        }
        const int64_t npix = (int64_t)r.oh * r.ow, pix = (int64_t)oy * r.ow + ox;
#pragma unroll
        for (int c = 0; c < PL; c++) {
            if (c >= n_out) continue;
            const int64_t e = t.layout == JXL_TENSOR_HWC ? pix * n_out + c : (int64_t)c * npix + pix;
            store_element<BYTES>(t.out, e, &q[c], 0);
        }
    }
    __syncthreads();  // (the next tile of this workgroup writes the image again)
}

}  // namespace jxl
#endif  // JXL_TENSOR_RESIZE_BODY_H
