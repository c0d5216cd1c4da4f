// Fused restoration + colour tile kernel for gfx950:
//   Gaborish -> EPF iteration(s) -> XYB->linear -> (transfer + quantise) in ONE launch, one read and
//   one write of the frame planes; all intermediates live in LDS.
//
// Replaces the same reference functions as k_restore.hip (Frame.java:505-679,
// OpsinInverseMatrix.java:105-142, JXLImage.java:244-258, ImageBuffer.java:129-147) and is checked
// bit-for-bit against them through the oracle AND against the stage kernels.
//
// Geometry (template <GAB, ITERS, SK, PH>): the most expensive stage -- the first EPF iteration that runs -- is computed on a
// 64x32 window = 512 threads x (4 wide x 1 tall) register patches (PH = 2: 256 threads x 4x2 patches, measured slower). Later
// iterations shrink the window by their radius (iteration 1: 2 px of input halo, iteration 2: 1, iteration 0: 3), Gaborish
// adds 1. E.g. the default (Gab + iterations 1,2): input tile 70x38 -> Gab 68x36 -> EPF1 64x32 -> EPF2 62x30 output tile.
// r5: a frame with three iterations runs as TWO launches (host.hip run_frame): ITERS = 4 -- Gaborish + the 13-tap iteration alone on a
// 64x64 tile, float planes out -- and ITERS = 2 without Gaborish from there; ITERS = 3 (all in one launch) stays for JXL_EPF3_SPLIT=0.
// ONE LDS image of 3 planes (~34 KB) that every stage updates IN PLACE: a thread computes the patch it owns into registers, the
// workgroup meets at a barrier (all reads of the old values done), then the patches are written back over the input
// (4 workgroups per CU = 8 waves per SIMD at 63 VGPRs).
//
// Exactness: per pixel the EPF distance is the reference's strictly sequential sum
//   dist = (((0 + |a-b|*s0) + ...)            channel-major, cross order (0,0),(0,-1),(0,1),(-1,0),(1,0)
// Every |P(u) - P(v)| * scale term is written with canonically ordered operands (|x-y| == |y-x| exactly)
// so the compiler's value numbering shares the terms between the pixels and taps of a patch instead of
// recomputing them. The centre tap has distance exactly 0 and weight exactly 1 for finite samples (the
// IDCT output is finite), so it is folded: sumWeights starts at 1, sumChannels at the centre sample.
// Frame edges: Gab reads clamped coordinates, EPF reads mirrored ones (MathHelper.mirrorCoordinate);
// edge tiles re-create that by copying mirrored positions inside LDS after each stage.
//
// This header holds the kernel template (restore_fused_body<GAB, ITERS, SK, PH>, SK = the output sink kind of restore_sink.h) and its
// launch templates; it is included by k_restore_fused.hip (float planes: the hot variants, and the public entry points),
// k_restore_fused_gen.hip (the run-time-generic sink) and k_restore_fused_q.hip (the quantised PNG / u16 sinks), so that the three
// groups of instantiations compile in parallel.
#pragma once
#include <hip/hip_ext.h>  // hipExtLaunchKernelGGL (a launch that records the kernel's own start / stop events)
#include "jxl_internal.h"
#include <algorithm>
#include "restore_sink.h"
#include "epf_quot3.h"
#include <cstdlib>
#include <type_traits>

namespace jxl {

#ifndef JXL_EPF3_PH2_WAVES
#define JXL_EPF3_PH2_WAVES 2
#endif

namespace {

__device__ __forceinline__ int mirror_c(int c, int size) {
    while (c < 0 || c >= size) {
        const int tc = ~c;
        c = tc >= 0 ? tc : (size << 1) + tc;
    }
    return c;
}

template <bool GAB, int ITERS>
struct Geo {
    static constexpr int RG = GAB ? 1 : 0;
    // ITERS = 4: the 13-tap iteration ALONE (the first half of a three-iteration frame run as two launches, k_restore_fused.hip)
    static constexpr int R0 = (ITERS == 3 || ITERS == 4) ? 3 : 0;
    static constexpr int R1 = (ITERS >= 1 && ITERS <= 3) ? 2 : 0;
    static constexpr int R2 = (ITERS == 2 || ITERS == 3) ? 1 : 0;
    static constexpr int SHR = ITERS == 3 ? (R1 + R2) : ITERS == 2 ? R2 : 0;  // window -> output tile
#ifndef JXL_EPF0_WH
#define JXL_EPF0_WH 64
#endif
    // the 13-tap iteration alone has no later stage to shrink for, and its 118 registers hold it to 2 workgroups per CU whatever the
    // tile costs in LDS: a 64 x 64 window (66 KB) loads and Gab-filters 1.27 x / 1.20 x its pixels instead of 1.41 x / 1.30 x
    static constexpr int WH = ITERS == 4 ? JXL_EPF0_WH : 32;                  // window height
    static constexpr int OW = 64 - 2 * SHR, OH = WH - 2 * SHR;               // output tile
    static constexpr int RE = R0 + R1 + R2;
    static constexpr int RT = RE + RG;                                        // input halo
    static constexpr int IW = OW + 2 * RT, IH = OH + 2 * RT;                  // input tile
    static constexpr int SW = IW + 3;                                         // LDS row stride (patch over-read <= 3)
    static constexpr int SH = IH + 1;
    static constexpr int PLANE = SW * SH;
    // behind the image and the sigma cells: the handoff area of the 5-tap iterations' pair chains (epf_stage). North part: 9 rows of
    // 64 chains -- row 0 from the edge pass, row w + 1 the south chains of wave w's bottom window row; west part: 5 columns of 32 --
    // column 0 from the edge pass, column k + 1 the east chains of patch column 4 k + 3. (The last row and column have no reader.)
    // 16-byte aligned: a patch takes its four north chains in one read.
    static constexpr bool HAND = R1 != 0 || R2 != 0;
    static constexpr int HOFF = (3 * PLANE + 16 * 16 + 3) & ~3;
    static constexpr int HNORTH = 9 * 64, HWEST = 5 * 32;
    static constexpr size_t LDS_BYTES = sizeof(float) * (HAND ? HOFF + HNORTH + HWEST : 3 * PLANE + 16 * 16);
};

// canonical |P[u] - P[v]| * s: operands ordered by index so equal terms are literally the same expression
template <int PS>
__device__ __forceinline__ float adiff(const float* p, int u, int v, float s) {
    return u < v ? fabsf(p[u] - p[v]) * s : fabsf(p[v] - p[u]) * s;
}

// The pair chains of a 4 x PH patch at (ry, rx), iterations 1 and 2 (epf_patch explains them and why they are exact):
//   hc[py][j] = distance between (py, j-1) and (py, j), j = 0..4;  vc[i][px] = between (i-1, px) and (i, px), i = 0..PH
// OWN = 1: only the chains to the east and south neighbours, j and i from 1 -- hc[.][0] and vc[0][.] are left as they are (the
// west and north chains are what the patches to the left and above form as THEIR east and south chains, epf_stage)
template <int ITER, int SW, int PLANE, int PH, int OWN>
__device__ __forceinline__ void epf_pair_chains(const float* __restrict__ src, int ry, int rx, const EpfParams& ep, float hc[PH][5],
                                                float vc[PH + 1][4]) {
    constexpr int R = ITER == 1 ? 2 : 1;
    constexpr int NW = 4 + 2 * R, NH = PH + 2 * R;
    constexpr int QY[5] = {0, 0, 0, -1, 1};
    constexpr int QX[5] = {0, -1, 1, 0, 0};
    auto chain_channel = [&](int c, auto first_channel) {
        constexpr bool FIRST = decltype(first_channel)::value;
        float nb[NH * NW];
        const float* pc = src + c * PLANE + (ry - R) * SW + (rx - R);
#pragma unroll
        for (int y = 0; y < NH; y++)
#pragma unroll
            for (int x = 0; x < NW; x++) nb[y * NW + x] = pc[y * SW + x];
        const float sc = ep.channel_scale[c];
#pragma unroll
        for (int py = 0; py < PH; py++)
#pragma unroll
            for (int j = OWN; j < 5; j++) {
                const int cy = py + R, cx = j - 1 + R;
                if (ITER == 2) {
                    const float t = adiff<NW>(nb, cy * NW + cx, cy * NW + cx + 1, sc);
                    hc[py][j] = FIRST ? t : hc[py][j] + t;
                } else
#pragma unroll
                    for (int q = 0; q < 5; q++) {
                        const int u = (cy + QY[q]) * NW + cx + QX[q];
                        const float t = adiff<NW>(nb, u, u + 1, sc);
                        hc[py][j] = (FIRST && q == 0) ? t : hc[py][j] + t;
                    }
            }
#pragma unroll
        for (int i = OWN; i <= PH; i++)
#pragma unroll
            for (int px = 0; px < 4; px++) {
                const int cy = i - 1 + R, cx = px + R;
                if (ITER == 2) {
                    const float t = adiff<NW>(nb, cy * NW + cx, (cy + 1) * NW + cx, sc);
                    vc[i][px] = FIRST ? t : vc[i][px] + t;
                } else
#pragma unroll
                    for (int q = 0; q < 5; q++) {
                        const int u = (cy + QY[q]) * NW + cx + QX[q];
                        const float t = adiff<NW>(nb, u, u + NW, sc);
                        vc[i][px] = (FIRST && q == 0) ? t : vc[i][px] + t;
                    }
            }
    };
    chain_channel(0, std::true_type{});
#pragma unroll 1
    for (int c = 1; c < 3; c++) chain_channel(c, std::false_type{});
}

// ONE pair chain, by the edge pass of epf_stage: the distance between (y, x) and its neighbour D floats further (D = 1: to the east,
// D = SW: to the south), the terms of epf_pair_chains in their order: channel-major, cross-minor, first minus second, started at the
// first term. Equal to hc[.][j] / vc[i][.] of any patch that holds the pair, bit for bit.
template <int ITER, int SW, int PLANE, int D>
__device__ __forceinline__ float epf_pair_chain(const float* __restrict__ src, int y, int x, const EpfParams& ep) {
    constexpr int QY[5] = {0, 0, 0, -1, 1};
    constexpr int QX[5] = {0, -1, 1, 0, 0};
    float d = 0.0f;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const float* p = src + c * PLANE + y * SW + x;
        const float sc = ep.channel_scale[c];
#pragma unroll
        for (int q = 0; q < (ITER == 2 ? 1 : 5); q++) {
            const int o = QY[q] * SW + QX[q];
            const float t = fabsf(p[o] - p[o + D]) * sc;
            d = (c == 0 && q == 0) ? t : d + t;
        }
    }
    return d;
}

// One EPF iteration (Frame.java:583-635) on a 4x2 patch whose top-left sample is (ry, rx) in region
// coordinates of src (3 planes, stride SW). Results for the 8 pixels go to res[c][py*4+px].
// ITER: 0 = 13 taps with cross distances, 1 = 5 taps with cross distances, 2 = 5 taps single-pixel.
// PLAINDIV: three plain divisions per pixel instead of epf_quot3_patch -- the form for parameter sets with a negative factor in the
// weights, whose sums of weights are not bounded (see the weights below; epf_weights_plain() chooses on the host).
template <int ITER, int SW, int PLANE, int PH, bool PLAINDIV = false, bool CHAINS = true, bool GIVEN = false>
__device__ __forceinline__ void epf_patch(const float* __restrict__ src, int ry, int rx, const float* s_inv /*[NP]*/,
                                          const float* bmul /*[NP]*/, const EpfParams& ep, float res[3][4 * PH],
                                          const float* given_h = nullptr /*[5]*/, const float* given_v = nullptr /*[2][4]*/) {
    constexpr int NP = 4 * PH;  // pixels per patch
    constexpr int R = ITER == 0 ? 3 : ITER == 1 ? 2 : 1;  // neighbourhood radius
    constexpr int NW = 4 + 2 * R, NH = PH + 2 * R;
    constexpr int NT = ITER == 0 ? 12 : 4;  // non-centre taps
    // (dy, dx) in the reference's order, centre tap folded (Frame.java:44-55)
    constexpr int TY[12] = {0, 0, -1, 1, -1, 1, 1, -1, 0, 0, 2, -2};
    constexpr int TX[12] = {-1, 1, 0, 0, 1, 1, -1, -1, -2, 2, 0, 0};
    constexpr int QY[5] = {0, 0, 0, -1, 1};
    constexpr int QX[5] = {0, -1, 1, 0, 0};

    float dist[NP][NT];
#pragma unroll
    for (int i = 0; i < NP; i++)
#pragma unroll
        for (int t = 0; t < NT; t++) dist[i][t] = 0.0f;

    if (ITER != 0 && CHAINS) {
        // The distance of pixel p to its east neighbour IS the distance of p+1 to its west neighbour: the same
        // terms |P(p+k) - P(p+1+k)| * s in the same channel-major, cross-minor order (likewise south/north). So a
        // patch needs one chain per horizontally / vertically adjacent pixel PAIR, not one per (pixel, tap):
        //   hc[py][j] = distance between (py, j-1) and (py, j), j = 0..4;  vc[i][px] = between (i-1, px) and (i, px), i = 0..PH
        //
        // A chain STARTS at its first term t0 = |a - b| * s instead of at 0 + t0 (the first channel is peeled off the channel loop for
        // that: no zero-filled accumulators, one add less per chain). Bit-identical where it can matter: 0 + t0 == t0 for every t0
        // but -0 (NaNs keep their payload through the add), and |a - b| * s is -0 only for s < 0 or s == -0 with a == b. The chain
        // then differs from the reference's only when EVERY term is a zero, and only in that zero's sign; the one use of a chain is
        // v = 1 - dist * bmul * sigma_scale * s_inv, where a zero of either sign gives the same product magnitude (0, or NaN if a
        // factor is not finite) and 1 - (+-0) is exactly 1. Every non-zero sum sees the same operands in the same order.
        //
        // GIVEN: the stage formed the chains already -- the patch's own to the east and south, the west and north ones taken from the
        // patches that formed them as theirs (epf_stage): the same pairs, so the same terms in the same order.
        float hc[PH][5], vc[PH + 1][4];
        if constexpr (GIVEN) {
            static_assert(PH == 1, "exchanged chains: 4x1 patches");
#pragma unroll
            for (int j = 0; j < 5; j++) hc[0][j] = given_h[j];
#pragma unroll
            for (int px = 0; px < 4; px++) vc[0][px] = given_v[px], vc[1][px] = given_v[4 + px];
        } else {
            epf_pair_chains<ITER, SW, PLANE, PH, 0>(src, ry, rx, ep, hc, vc);
        }
#pragma unroll
        for (int py = 0; py < PH; py++)
#pragma unroll
            for (int px = 0; px < 4; px++) {
                dist[py * 4 + px][0] = hc[py][px];      // tap (0,-1)
                dist[py * 4 + px][1] = hc[py][px + 1];  // tap (0,+1)
                dist[py * 4 + px][2] = vc[py][px];      // tap (-1,0)
                dist[py * 4 + px][3] = vc[py + 1][px];  // tap (+1,0)
            }
    } else {
    // 13-tap iteration: the four taps on the patch's own row -- (0,-1), (0,1), (0,-2), (0,2) -- are pair distances that two pixels of
    // the 4x1 patch share (dist(p, p + t) and dist(p + t, p) are the same terms in the same order): 5 + 6 chains instead of 16.
    // The other eight taps pair a pixel with one of another row, i.e. of another thread's patch.
    constexpr bool HROW = ITER == 0 && CHAINS && PH == 1;
    float h1[5], h2[6];
#pragma unroll
    for (int j = 0; j < 5; j++) h1[j] = 0.0f;
#pragma unroll
    for (int j = 0; j < 6; j++) h2[j] = 0.0f;
    // channels one after the other (not interleaved by the scheduler): keeps the live set under 128 VGPRs
#pragma unroll 1
    for (int c = 0; c < 3; c++) {
        // neighbourhood of this channel in registers; only the diamond of radius R around the patch is
        // ever referenced, the compiler drops the unused corner loads
        float nb[NH * NW];
        const float* pc = src + c * PLANE + (ry - R) * SW + (rx - R);
#pragma unroll
        for (int y = 0; y < NH; y++)
#pragma unroll
            for (int x = 0; x < NW; x++) nb[y * NW + x] = pc[y * SW + x];
        const float sc = ep.channel_scale[c];
#pragma unroll
        for (int py = 0; py < PH; py++)
#pragma unroll
            for (int px = 0; px < 4; px++) {
                const int cy = py + R, cx = px + R;  // centre inside nb
#pragma unroll
                for (int t = 0; t < NT; t++) {
                    if (HROW && TY[t] == 0) continue;  // through h1 / h2 below
                    if (ITER == 2) {  // epfDistance2 (:657-669): single pixel
                        dist[py * 4 + px][t] =
                            dist[py * 4 + px][t] + adiff<NW>(nb, cy * NW + cx, (cy + TY[t]) * NW + cx + TX[t], sc);
                    } else {  // epfDistance1 (:638-655): 5-point cross
#pragma unroll
                        for (int q = 0; q < 5; q++) {
                            const int u = (cy + QY[q]) * NW + cx + QX[q];
                            const int v = (cy + TY[t] + QY[q]) * NW + cx + TX[t] + QX[q];
                            dist[py * 4 + px][t] = dist[py * 4 + px][t] + adiff<NW>(nb, u, v, sc);
                        }
                    }
                }
            }
        if (HROW) {
            constexpr int cy = R;
#pragma unroll
            for (int j = 0; j < 5; j++)
#pragma unroll
                for (int q = 0; q < 5; q++) {
                    const int u = (cy + QY[q]) * NW + (j - 1 + R) + QX[q];
                    h1[j] = h1[j] + adiff<NW>(nb, u, u + 1, sc);
                }
#pragma unroll
            for (int j = 0; j < 6; j++)
#pragma unroll
                for (int q = 0; q < 5; q++) {
                    const int u = (cy + QY[q]) * NW + (j - 2 + R) + QX[q];
                    h2[j] = h2[j] + adiff<NW>(nb, u, u + 2, sc);
                }
        }
    }
    if (HROW) {
#pragma unroll
        for (int px = 0; px < 4; px++)
#pragma unroll
            for (int t = 0; t < NT; t++) {
                if (TY[t] != 0) continue;
                dist[px][t] = TX[t] == -1 ? h1[px] : TX[t] == 1 ? h1[px + 1] : TX[t] == -2 ? h2[px] : h2[px + 2];
            }
    }
    }
    // weights (epfWeight, :671-679), in place of the distances
    float sumW[NP];
    bool skip[NP];
#pragma unroll
    for (int i = 0; i < NP; i++) {
        const float s = s_inv[i];
        skip[i] = (s != s) || (s > (1.0f / 0.3f));  // :608-612
        float sw = 0.0f + 1.0f;                     // centre tap: dist 0 -> weight 1 (finite samples)
#pragma unroll
        for (int t = 0; t < NT; t++) {
            const float d = dist[i][t] * bmul[i];
            const float v = 1.0f - d * ep.sigma_scale * s;
            // max(v, 0): the reference's `v < 0 ? 0 : v` (Frame.java:676-678) for every v that is not NaN or -0. v = 1 - x is -0 for no x,
            // and NaN only where inv sigma is not finite or the samples are not -- skipped pixels, whose result is their centre sample
            // whatever their weights (the `skip` select of the plain divisions; on the fast path a NaN weight clamps to 0, see there).
            // x = dist * bmul * sigma_scale * s is >= 0 or NaN when channel_scale[], border_sad_mul, sigma_scale and the inverse sigma
            // are not negative (epf_weights_plain() is false: the !PLAINDIV instantiations), so every weight lies in [0, 1] and
            // 1 <= sumW <= 1 + NT for EVERY pixel, skipped ones included (their weights are formed like any other before the select
            // drops the result) -- what epf_quot3_patch needs of its denominators.
            // !PLAINDIV: v <= 1 or NaN, so min(max(v, 0), 1) == max(v, 0) bit for bit (for NaN both give 0: v_max_f32 is maxnum, and the
            // code objects run with DX10_CLAMP); hipcc folds that form into the subtraction's clamp output modifier and the half-rate
            // v_max_f32 goes
            const float w = !PLAINDIV ? __builtin_fminf(__builtin_fmaxf(v, 0.0f), 1.0f) : __builtin_fmaxf(v, 0.0f);
            dist[i][t] = w;
            sw = sw + w;
        }
        sumW[i] = sw;
    }
    // weighted sums per channel (:615-626): tap radius RT2 only
    constexpr int RT2 = ITER == 0 ? 2 : 1;
    constexpr int MW = 4 + 2 * RT2, MH = PH + 2 * RT2;
    if constexpr (!PLAINDIV) {
        // the twelve numerators of the patch first, then the quotients: three per pixel by its one denominator (epf_quot3.h)
        float num[3][NP];
#pragma unroll
        for (int c = 0; c < 3; c++) {
            float nb[MH * MW];
            const float* pc = src + c * PLANE + (ry - RT2) * SW + (rx - RT2);
#pragma unroll
            for (int y = 0; y < MH; y++)
#pragma unroll
                for (int x = 0; x < MW; x++) nb[y * MW + x] = pc[y * SW + x];
#pragma unroll
            for (int py = 0; py < PH; py++)
#pragma unroll
                for (int px = 0; px < 4; px++) {
                    const int i = py * 4 + px;
                    const int cy = py + RT2, cx = px + RT2;
                    float sc = 0.0f + nb[cy * MW + cx] * 1.0f;
#pragma unroll
                    for (int t = 0; t < NT; t++) sc = sc + nb[(cy + TY[t]) * MW + cx + TX[t]] * dist[i][t];
                    num[c][i] = sc;
                }
        }
        // A skipped pixel (:608-612) needs no select here. Its inverse sigma arrives as s = +inf (the window load of
        // restore_fused_body makes every NaN and every value above 1 / 0.3f that), and with no negative factor in the weights:
        //   x = d * sigma_scale * s is +inf or NaN (d >= 0 or NaN; 0 * inf is NaN), v = 1 - x is -inf or NaN, and the clamped weight is
        //   exactly +0 (maxnum and DX10_CLAMP, as above) for every tap;  sumW = 1 + 0 + ... is exactly 1, inside epf_quot3_patch's window;
        //   the numerator is (0 + centre * 1) + nb * 0 + ..., i.e. centre + (+-0) + ... = centre bit for bit when the centre is
        //   not +-0 and every neighbour is finite;  and epf_quot_by(n, 1, 1) is n (r0 = r1 = 1, every error term 0).
        // Where that fails -- a centre that is +-0 (numerator +0 whatever its sign) or a neighbour that is not finite (nb * 0 is NaN) -- the
        // numerator is 0 or NaN, outside the guard's window [2^-100, 2^90], and the whole wave takes the plain divisions, where the
        // select stays: its predicate holds for +inf. (Denormal and huge centres go there too, as they always did.)
        epf_quot3_patch<NP>(num, sumW, res, [&](int c, int i, float q) {
            const float s = s_inv[i];
            return ((s != s) || (s > (1.0f / 0.3f))) ? src[c * PLANE + (ry + i / 4) * SW + rx + i % 4] : q;
        });
        return;
    }
#pragma unroll
    for (int c = 0; c < 3; c++) {
        float nb[MH * MW];
        const float* pc = src + c * PLANE + (ry - RT2) * SW + (rx - RT2);
#pragma unroll
        for (int y = 0; y < MH; y++)
#pragma unroll
            for (int x = 0; x < MW; x++) nb[y * MW + x] = pc[y * SW + x];
#pragma unroll
        for (int py = 0; py < PH; py++)
#pragma unroll
            for (int px = 0; px < 4; px++) {
                const int i = py * 4 + px;
                const int cy = py + RT2, cx = px + RT2;
                float sc = 0.0f + nb[cy * MW + cx] * 1.0f;
#pragma unroll
                for (int t = 0; t < NT; t++) sc = sc + nb[(cy + TY[t]) * MW + cx + TX[t]] * dist[i][t];
#ifdef JXL_EPF_DIV_BRANCH
                res[c][i] = skip[i] ? nb[cy * MW + cx] : sc / sumW[i];
#else
                // the quotient is formed unconditionally (the empty asm keeps the optimiser from sinking the division into
                // a branch on `skip`): twelve exec-masked blocks per stage become straight-line code, and the schedulers
                // interleave the twelve dependent rcp / fma chains
                float qv = sc / sumW[i];
                asm volatile("" : "+v"(qv));
                res[c][i] = skip[i] ? nb[cy * MW + cx] : qv;
#endif
            }
    }
}

struct TileCtx {
    int ix0, iy0;  // frame coordinates of region (0,0)
    int W, H;
    bool edge;
};

// s_inv / border factor of the 4 x PH pixels of a patch
// EDGE = false: the path of interior tiles (whole input tile inside the frame): no coordinate clamps
template <int PH, bool EDGE>
__device__ __forceinline__ void patch_sigma(int ry, int rx, const TileCtx& tc, const float* __restrict__ sig, int scy0, int scx0,
                                            const EpfParams& ep, float s_inv[4 * PH], float bmul[4 * PH]) {
    const int gx0 = tc.ix0 + rx;
    // a 4-pixel run touches at most two cells: look up the first and the last, pick per pixel. Out-of-frame
    // positions (only on edge tiles: a uniform branch) get some in-range cell; they are recomputed by the mirror fix-up.
    int cxa = (gx0 >> 3) - scx0, cxb = ((gx0 + 3) >> 3) - scx0;
    if (EDGE) {
        cxa = (min(max(gx0, 0), tc.W - 1) >> 3) - scx0;
        cxb = (min(max(gx0 + 3, 0), tc.W - 1) >> 3) - scx0;
    }
    // pixel i of the run lies in the first cell while i < 8 - (gx0 & 7); it is on an 8x8-border column when (gx0 + i) & 7 is 0 or 7:
    // bit i of 0x8181 >> (gx0 & 7)
    const int first_n = 8 - (gx0 & 7);
    const uint32_t colb = 0x8181u >> (gx0 & 7);
#pragma unroll
    for (int py = 0; py < PH; py++) {
        const int gy = tc.iy0 + ry + py;
        const bool rowb = ((gy + 1) & 7) < 2;  // gy & 7 is 7 or 0
        int crow = ((gy >> 3) - scy0) * 16;
        if (EDGE) crow = ((min(max(gy, 0), tc.H - 1) >> 3) - scy0) * 16;
        const float sa = sig[crow + cxa], sb = sig[crow + cxb];
        const uint32_t bm = rowb ? 0xfu : colb;
#pragma unroll
        for (int px = 0; px < 4; px++) {
            // epfWeight's border factor (:672-675): border_sad_mul on 8x8-border rows/columns, else 1 (d * 1 == d)
            bmul[py * 4 + px] = (bm & (1u << px)) ? ep.border_sad_mul : 1.0f;
            s_inv[py * 4 + px] = px < first_n ? sa : sb;
        }
    }
}

// run one EPF iteration over the output region [m, IH-m) x [m, IW-m) of the tile.
// LAST: results go to the sink (colour + global store). Otherwise IN PLACE: every thread computes the one patch it owns
// into registers, the workgroup meets at a barrier (all reads of the old values done), then the patches are written
// back over the input. One LDS buffer instead of two doubles the workgroups a CU can hold.
template <int ITER, typename G, bool LAST, int PH, bool EDGE, bool PLAINDIV, typename Sink>
__device__ __forceinline__ void epf_stage(float* buf, int m, const TileCtx& tc, const float* __restrict__ sig, int scy0, int scx0,
                                          const EpfParams& ep, Sink sink) {
    constexpr int SW = G::SW, PLANE = G::PLANE;
    const int rw = G::IW - 2 * m, rh = G::IH - 2 * m;
    constexpr int NTHR = 512 / PH;
    const int pcols = (rw + 3) >> 2, prows = (rh + PH - 1) / PH;
    if constexpr (PH == 1 && ITER != 0) {
        // 5-tap iterations on 4x1 patches: EVERY PAIR CHAIN OF THE WINDOW IS FORMED ONCE. A thread forms the four chains of its
        // pixels to their south neighbours and the four to their east neighbours (epf_pair_chains, OWN); its north chains are the
        // south chains of the patch above and its west chain is the last east chain of the patch to the left -- the same pixel
        // pairs, hence the same terms |P(u) - P(v)| * s with the same first and second operand in the same channel-major,
        // cross-minor order, started at the same first term: the same bits (the argument of epf_patch, applied across patches).
        // On edge tiles every chain is formed from the LDS image as mirror_fixup left it, so this holds on mirrored rows and
        // columns as well. Weights, sums, quotients and sinks are untouched.
        //
        // thread -> patch: a wave is 4 window rows x 16 patch columns (wave w: rows 4 w .. 4 w + 3), and each 16-lane DPP row of it is
        // a 4 x 4 block of patches, lane = 4 * row + column. A 32-lane half is then still 8 patches x 4 rows, so the bank argument
        // below holds as it stands. The chains travel
        //   * inside a 4 x 4 block by DPP: north from the lane one row up (row_shr:4), west from the lane to the left (quad_perm);
        //   * across blocks and waves through the handoff area (Geo::HOFF): the bottom row of every wave writes its south chains, every
        //     fourth patch column its last east chain;
        //   * for the window's own top row and left column from the edge pass: ONE wave forms those 64 + 32 chains, one per lane, from
        //     the halo that is in LDS anyway (radius 2 / 1 around the region: inside the input tile since m >= the radius).
        // One more barrier per stage separates "chains formed and handed off" from "weights". Lanes that DPP serves ignore what they
        // read from the handoff area (row_shr writes only lanes with a source in their DPP row; the others keep `old`).
        // (!HAND: Geo<., 4>, whose one iteration is the 13-tap one -- instantiated by restore_epf_stages' plain `if`s, never run)
        static_assert(!G::HAND || (G::OW > 48 && G::WH == 32 && NTHR == 512), "13..16 patch columns, 32 window rows on 8 waves");
        extern __shared__ __attribute__((aligned(16))) float lds[];
        float* const hnorth = lds + G::HOFF;
        float* const hwest = hnorth + G::HNORTH;
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        const int pcol = ((lane >> 4) << 2) + (lane & 3), prow = (wave << 2) + ((lane >> 2) & 3);
        const bool act = prow < prows && pcol < pcols;
        const int ry = m + prow, rx = m + pcol * 4;
        // A lane without a patch of the region (rows 30, 31 and the like) still owns one of the 64 x 32 window, and forms it like any
        // other where all that this reads lies inside the LDS image (`whole`: a constant once m is known, true for every stage of
        // every variant -- the spare row IH and the pad columns included): nothing but its store is masked, so no value that
        // crosses a barrier needs a defined content for masked lanes. What such a lane hands on feeds dropped results only.
        constexpr int R = ITER == 1 ? 2 : 1;
        // (Not with the plain divisions: unmasked, their two-iteration variants spill 12 bytes; masked they hold 64 registers.)
        const bool whole = !PLAINDIV && m + 31 + R <= G::IH && m + 63 + R <= G::IW + 2;
        float s_inv[4], bmul[4];
        float hc[5], vc[2][4];
        if (whole || act) {
            patch_sigma<1, EDGE>(ry, rx, tc, sig, scy0, scx0, ep, s_inv, bmul);
            float (*h1)[5] = reinterpret_cast<float (*)[5]>(hc);
            epf_pair_chains<ITER, SW, PLANE, 1, 1>(buf, ry, rx, ep, h1, vc);
            if ((lane & 12) == 12) {
                float* d = hnorth + (wave + 1) * 64 + pcol * 4;
                *reinterpret_cast<float4*>(d) = make_float4(vc[1][0], vc[1][1], vc[1][2], vc[1][3]);
            }
            if ((lane & 3) == 3) hwest[((pcol >> 2) + 1) * 32 + prow] = hc[4];
        }
        // the edge pass (its two halves on two waves measured the same: profiles/restore_chain_once.md)
        if (__builtin_amdgcn_readfirstlane(wave) == NTHR / 64 - 1) {
            if (lane < rw) hnorth[lane] = epf_pair_chain<ITER, SW, PLANE, SW>(buf, m - 1, m + lane, ep);
            if (lane < rh) hwest[lane] = epf_pair_chain<ITER, SW, PLANE, 1>(buf, m + lane, m - 1, ep);
        }
        __syncthreads();
        float res[3][4];
        if (whole || act) {
            const float4 n4 = *reinterpret_cast<const float4*>(hnorth + wave * 64 + pcol * 4);
            const float w1 = hwest[(pcol >> 2) * 32 + prow];
            const float nn[4] = {n4.x, n4.y, n4.z, n4.w};
            // update_dpp(old, src, ctrl, row mask, bank mask, bound_ctrl = false): 0x114 = row_shr:4; a lane of the block's top row has
            // no source and keeps `old`, what it read from the handoff area
#pragma unroll
            for (int px = 0; px < 4; px++)
                vc[0][px] = __int_as_float(
                    __builtin_amdgcn_update_dpp(__float_as_int(nn[px]), __float_as_int(vc[1][px]), 0x114, 0xf, 0xf, false));
            // west: quad_perm:[0,0,1,2] (0x90) -- a quad is one row of the block, every lane takes the chain of the lane to its left,
            // the first lane of the quad its own, for which the handoff value stands in
            const float wl = __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(hc[4]), 0x90, 0xf, 0xf, true));
            hc[0] = (lane & 3) == 0 ? w1 : wl;
            epf_patch<ITER, SW, PLANE, 1, PLAINDIV, true, true>(buf, ry, rx, s_inv, bmul, ep, res, hc, &vc[0][0]);
        }
        if constexpr (LAST) {
            if (act) sink.row4(ry, rx, &res[0][0], &res[1][0], &res[2][0], min(4, G::IW - m - rx));
        } else {
            __syncthreads();
            if (act) {
#pragma unroll
                for (int px = 0; px < 4; px++) {
                    const int x = rx + px;
                    if (x < G::IW - m) {
#pragma unroll
                        for (int c = 0; c < 3; c++) buf[c * PLANE + ry * SW + x] = res[c][px];
                    }
                }
            }
        }
        return;
    }
    // thread -> patch. LDS banks are (address / 4) mod 32 for ds_read_b32 / ds_read2 / ds_write, and lanes conflict within a
    // 32-lane half. A patch is 4 floats wide, so 16 patches of one row put their first words on only 8 banks: the row-major
    // assignment (lane -> 16 patches x 2 rows) made every tap read and every write-back a 2-way conflict (44 % of all LDS
    // cycles, profiles/r1). With 8 patches x 4 rows per half the rows add 0, SW, 2 SW, 3 SW: SW is odd, so they land in the
    // four residue classes mod 4 and the 32 lanes cover the 32 banks exactly once. Any constant tap offset keeps that.
    const int cblocks = (pcols + 7) >> 3, n_groups = cblocks * ((prows + 3) >> 2);
    const int q = threadIdx.x & 31;
    auto patch_of = [&](int g, int& prow, int& pcol) {
        pcol = (g % cblocks) * 8 + (q & 7);
        prow = (g / cblocks) * 4 + (q >> 3);
        return prow < prows && pcol < pcols;
    };
    if (LAST) {
        for (int g = threadIdx.x >> 5; g < n_groups; g += NTHR / 32) {
            int prow, pcol;
            if (!patch_of(g, prow, pcol)) continue;
            const int ry = m + prow * PH, rx = m + pcol * 4;
            float s_inv[4 * PH], bmul[4 * PH];
            patch_sigma<PH, EDGE>(ry, rx, tc, sig, scy0, scx0, ep, s_inv, bmul);
            float res[3][4 * PH];
            epf_patch<ITER, SW, PLANE, PH, PLAINDIV>(buf, ry, rx, s_inv, bmul, ep, res);
#pragma unroll
            for (int py = 0; py < PH; py++) {
                const int y = ry + py;
                if (y < G::IH - m) sink.row4(y, rx, &res[0][py * 4], &res[1][py * 4], &res[2][py * 4], min(4, G::IW - m - rx));
            }
        }
    } else {
        // the largest region any stage sees is the 64x32 window: one patch per thread
        static_assert((64 / 4) * ((32 + PH - 1) / PH) <= NTHR, "one patch per thread");
        int prow, pcol;
        const bool act = patch_of(threadIdx.x >> 5, prow, pcol);  // 16 groups of 8 x 4 patches cover the 16 x 32 window
        const int ry = m + prow * PH, rx = m + pcol * 4;
        float res[3][4 * PH];
        if (act) {
            float s_inv[4 * PH], bmul[4 * PH];
            patch_sigma<PH, EDGE>(ry, rx, tc, sig, scy0, scx0, ep, s_inv, bmul);
            epf_patch<ITER, SW, PLANE, PH, PLAINDIV>(buf, ry, rx, s_inv, bmul, ep, res);
        }
        __syncthreads();
        if (act) {
#pragma unroll
            for (int py = 0; py < PH; py++) {
                const int y = ry + py;
#pragma unroll
                for (int px = 0; px < 4; px++) {
                    const int x = rx + px;
                    if (y < G::IH - m && x < G::IW - m) {
#pragma unroll
                        for (int c = 0; c < 3; c++) buf[c * PLANE + y * SW + x] = res[c][py * 4 + px];
                    }
                }
            }
        }
    }
}

// after a non-final stage on an edge tile: positions of the region outside the frame take the value of
// their mirrored in-frame position (what a mirrored read of the full-frame plane would return)
template <typename G, int NTHR>
__device__ __forceinline__ void mirror_fixup(float* __restrict__ buf, int m, int rem, const TileCtx& tc) {
    const int rw = G::IW - 2 * m, rh = G::IH - 2 * m;
    __syncthreads();
    for (int i = threadIdx.x; i < rw * rh; i += NTHR) {
        const int y = m + i / rw, x = m + i % rw;
        const int gy = tc.iy0 + y, gx = tc.ix0 + x;
        const bool outside = gy < 0 || gy >= tc.H || gx < 0 || gx >= tc.W;
        // only positions within the radius the remaining stages can reach from an in-frame pixel matter
        const bool near = gy >= -rem && gy < tc.H + rem && gx >= -rem && gx < tc.W + rem;
        if (outside && near) {
            const int my = mirror_c(gy, tc.H) - tc.iy0, mx = mirror_c(gx, tc.W) - tc.ix0;
#pragma unroll
            for (int c = 0; c < 3; c++) buf[c * G::PLANE + y * G::SW + x] = buf[c * G::PLANE + my * G::SW + mx];
        }
    }
}


typedef float v2f_t __attribute__((ext_vector_type(2)));
struct __attribute__((packed, aligned(4))) f2a4 {
    float x, y;
};

// OpsinInverseMatrix.invertXYB + JXLImage.transferInPlace + ImageBuffer.castToInt0 + the global store; SK = sink kind (restore_sink.h)
// EDGE = false: every position handed over lies inside the frame (interior tiles), so the frame-bound tests go
template <int SK, bool NT = false, bool EDGE = true>
struct OutSink {
    const FusedArgs& a;
    const TileCtx& tc;
    __device__ __forceinline__ void colour(float& v0, float& v1, float& v2) const {
        if (a.p.xyb) invert_xyb_px(a.p.xybp, v0, v1, v2);
    }
    // one pixel at region position (y, x)
    __device__ __forceinline__ void operator()(int y, int x, float v0, float v1, float v2) const {
        const int gy = tc.iy0 + y, gx = tc.ix0 + x;
        if (EDGE && (gy >= tc.H || gx >= tc.W)) return;
        colour(v0, v1, v2);
        sink_store_k<SK>(a, (uint32_t)(gy * tc.W + gx), v0, v1, v2);
    }
    // up to 4 consecutive pixels of a row (a patch row)
    __device__ __forceinline__ void row4(int y, int x, const float* r0, const float* r1, const float* r2, int nvalid) const {
        const int gy = tc.iy0 + y, gx = tc.ix0 + x;
        if (EDGE && gy >= tc.H) return;
        const int n = EDGE ? min(nvalid, tc.W - gx) : nvalid;
        if (n <= 0) return;
        float o[3][4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            o[0][i] = r0[i];
            o[1][i] = r1[i];
            o[2][i] = r2[i];
            colour(o[0][i], o[1][i], o[2][i]);
        }
        const uint32_t g = (uint32_t)(gy * tc.W + gx);
        // a whole run of 4 from an even pixel index (tile origins are multiples of 62 px, patch columns of 4, frame widths of 8:
        // g is even for every full run): the kind's wide stores
        if (n == 4 && (g & 1u) == 0 && sink_store4_k<SK, NT>(a, g, o)) return;
#pragma unroll
        for (int i = 0; i < 4; i++)
            if (i < n) sink_store_k<SK>(a, g + i, o[0][i], o[1][i], o[2][i]);
    }
};

template <bool GAB, int ITERS, int SK, int PH, bool EDGE, bool PLAINDIV>
__device__ __forceinline__ void restore_epf_stages(const FusedArgs& a, float* cur, int m, const TileCtx& tc, const float* __restrict__ sig,
                                                   int scy0, int scx0);

// SK = SK_PLAIN: float planes out, no transfer function (keeps the transfer code out of the hot variant); the other sink kinds
// fix transfer function and output format at compile time, SK_GENERIC picks them per sample at run time
// LAY = the layout of the input planes: 0 raster, 1 cell-tiled (plane_tiled.h: run_frame's pooled planes, written by the IDCT launch of
// the same call). Only the tile load differs: both loaders leave the same LDS image.
template <bool GAB, int ITERS, int SK, int PH, int LAY = 0, bool PLAINDIV = false>
__device__ __forceinline__ void restore_fused_body(const FusedArgs& a) {
    using G = Geo<GAB, ITERS>;
    constexpr int NTHR = 512 / PH;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    // cell-tiled input: the tile starts three floats into the allocation, so that the whole-piece loader below may write up to three
    // samples in front of row 0 of the first plane. LDS_BYTES does not grow for it: the tile's last three floats -- pad columns of
    // the third plane's spare row IH, which no loader and no write-back reaches -- now lie over the first three sigma cells, and
    // are as before only ever read, by a patch's over-read, for results that are dropped. (The sigma window in front of the tile
    // would serve too -- its row 15 is never read --, but a base of 1 KiB takes the paired LDS reads of the EPF stages out of their
    // immediate range: +21 address instructions per thread, counted; three floats cost 3.)
    constexpr int FRONT = LAY == 1 ? 3 : 0;
    float* A = lds + FRONT;           // the tile: 3 planes, every stage works in place
    float* sig = lds + 3 * G::PLANE;  // [16][16] inverse sigma of the cells under the tile
    const int W = a.W, H = a.H;
    TileCtx tc;
    tc.W = W;
    tc.H = H;
    // XCD-aware tile order: workgroups are dealt round-robin over the 8 XCDs (b % 8 share an L2), so give every
    // XCD one contiguous run of tiles in raster order: neighbouring tiles (shared halo reads, shared 128-byte
    // lines of the 62-wide output rows) then meet in the same L2. Speed only, never correctness.
    const int tiles_x = (W + G::OW - 1) / G::OW, tiles_y = (H + G::OH - 1) / G::OH;
    int ox, oy;
    {
        const int n_tiles = tiles_x * tiles_y;
        const int per_xcd = (n_tiles + 7) >> 3;
        const int tile = (int)(blockIdx.x & 7u) * per_xcd + (int)(blockIdx.x >> 3);
        if (tile >= n_tiles) return;  // uniform per workgroup, before any barrier
        ox = (tile % tiles_x) * G::OW;
        oy = (tile / tiles_x) * G::OH;
    }
    tc.ix0 = ox - G::RT;
    tc.iy0 = oy - G::RT;
    tc.edge = tc.ix0 < 0 || tc.iy0 < 0 || tc.ix0 + G::IW > W || tc.iy0 + G::IH > H;

    // inverse sigma per cell (Frame.java:552-571): a constant of the frame, formed once per frame description (host.hip:
    // build_inv_sigma, or k_epf_sigma where the maps arrive as device planes) -- the window under the tile is only loaded
    const int scy0 = max(tc.iy0, 0) >> 3, scx0 = max(tc.ix0, 0) >> 3;
    if (ITERS > 0 && threadIdx.x < 256) {
        const int cy = scy0 + (threadIdx.x >> 4), cx = scx0 + (threadIdx.x & 15);
        float v = 0.0f;
        if (cy < ((H + 7) >> 3) && cx < a.bw) v = a.inv_sigma[cy * a.bw + cx];
        // every cell the reference skips (:608-612: NaN, or above 1 / 0.3f) as +inf, whichever producer wrote the plane: the
        // skip rule holds for +inf as for the value it replaces, and the fast-division tails of epf_patch rely on the infinity
        if (v != v || v > (1.0f / 0.3f)) v = __builtin_inff();
        sig[threadIdx.x] = v;
    }
    // load the input tile: clamped coordinates feed Gab, mirrored ones feed EPF directly. Flat row-major
    // walk with incrementally updated (y, x) and 32-bit plane offsets (scalar base + 32-bit lane offset).
    if (LAY == 1 && !tc.edge) {
        // interior tile of cell-tiled planes: the tile is gathered from the NCY x NCX cells it can overlap (6 x 10 for the 70 x 38 tile),
        // 16 consecutive lanes = the 16 aligned 16-byte pieces of one cell = two whole 128-byte lines. A piece outside the tile is not
        // loaded (for an interior tile everything inside it lies inside the frame).
        constexpr int NCX = (G::IW + 6) / 8 + 1, NCY = (G::IH + 6) / 8 + 1, TOTAL = NCX * NCY * 16;
        const int cells_w = W >> 3;
        const int ccy0 = tc.iy0 >> 3, ccx0 = tc.ix0 >> 3;
        // A piece that straddles the tile's left or right edge is stored WHOLE, like every other: no test per sample. Its samples
        // outside the tile land in the row's pad columns IW .. IW + 2 (SW = IW + 3): up to three past the right edge in the piece's own
        // row, up to three in front of column 0 at the end of the row above -- for row 0 of the first plane those are the three floats
        // in front of the tile (FRONT), for the other planes the spare row IH of the plane in front.
        // Nobody reads a pad column's value: Gaborish reads columns 0 .. IW - 1, and what an EPF patch reads past its region feeds
        // only results that are dropped. So it does not matter either that the pieces of two rows may write different garbage to the
        // same pad word in any order.
        // The lane's pieces are NTHR / 16 cells apart: cell row, cell column, coordinates and offset advance by constants.
        static_assert(NTHR % 16 == 0, "a lane keeps its piece index");
        constexpr int CSTEP = NTHR / 16, DY = CSTEP / NCX, DX = CSTEP % NCX;
        const int pc = threadIdx.x & 15;
        const int cyi0 = (int)(threadIdx.x >> 4) / NCX;
        int cxi = (int)(threadIdx.x >> 4) - cyi0 * NCX;
        int y = ((ccy0 + cyi0) << 3) + (pc >> 1) - tc.iy0, x = ((ccx0 + cxi) << 3) + ((pc & 1) << 2) - tc.ix0;  // tile coordinates
        // the address: a workgroup-uniform base per plane (the tile's first cell; 64-bit scalar arithmetic) + the lane's BYTE offset
        // from there in 32 bits (under NCY x cells_w cells of 256 bytes), which is the form a global load takes a scalar base in
        const size_t tile0 = (size_t)(uint32_t)(ccy0 * cells_w + ccx0) << 6;
        const char* const in0 = reinterpret_cast<const char*>(a.in[0] + tile0);
        const char* const in1 = reinterpret_cast<const char*>(a.in[1] + tile0);
        const char* const in2 = reinterpret_cast<const char*>(a.in[2] + tile0);
        uint32_t g = ((uint32_t)(cyi0 * cells_w + cxi) << 8) + (uint32_t)(pc << 4);
        const uint32_t gstep = (uint32_t)(DY * cells_w + DX) << 8, gwrap = (uint32_t)(cells_w - NCX) << 8;
#pragma unroll
        for (int k = 0; k < (TOTAL + NTHR - 1) / NTHR; k++) {
            // (a piece index past TOTAL lies in cell row NCY, whose y is past the tile: 8 NCY - 7 >= IH)
            if ((unsigned)y < (unsigned)G::IH && (unsigned)(x + 3) < (unsigned)(G::IW + 3)) {
                const float4 v0 = *reinterpret_cast<const float4*>(in0 + g);
                const float4 v1 = *reinterpret_cast<const float4*>(in1 + g);
                const float4 v2 = *reinterpret_cast<const float4*>(in2 + g);
                float* d = A + y * G::SW + x;
                d[0] = v0.x, d[1] = v0.y, d[2] = v0.z, d[3] = v0.w;
                d[G::PLANE] = v1.x, d[G::PLANE + 1] = v1.y, d[G::PLANE + 2] = v1.z, d[G::PLANE + 3] = v1.w;
                d[2 * G::PLANE] = v2.x, d[2 * G::PLANE + 1] = v2.y, d[2 * G::PLANE + 2] = v2.z, d[2 * G::PLANE + 3] = v2.w;
            }
            cxi += DX;
            y += 8 * DY;
            x += 8 * DX;
            g += gstep;
            if (cxi >= NCX) {
                cxi -= NCX;
                y += 8;
                x -= 8 * NCX;
                g += gwrap;
            }
        }
    } else if (!tc.edge) {
        // interior tile: no coordinate fix-ups; two samples per lane and load (the tile origin is only 4-byte aligned)
        static_assert(G::IW % 2 == 0, "pairs");
        constexpr int PAIRS = G::IW / 2, TOTAL = PAIRS * G::IH;
        const uint32_t base = (uint32_t)(tc.iy0 * W + tc.ix0);
#pragma unroll
        for (int k = 0; k < (TOTAL + NTHR - 1) / NTHR; k++) {
            const int idx = (int)threadIdx.x + k * NTHR;
            if (idx < TOTAL) {
                const int y = idx / PAIRS, x = (idx - y * PAIRS) * 2;
                const uint32_t g = base + (uint32_t)(y * W + x);
                const f2a4 v0 = *reinterpret_cast<const f2a4*>(a.in[0] + g);
                const f2a4 v1 = *reinterpret_cast<const f2a4*>(a.in[1] + g);
                const f2a4 v2 = *reinterpret_cast<const f2a4*>(a.in[2] + g);
                float* d = A + y * G::SW + x;
                d[0] = v0.x;
                d[1] = v0.y;
                d[G::PLANE] = v1.x;
                d[G::PLANE + 1] = v1.y;
                d[2 * G::PLANE] = v2.x;
                d[2 * G::PLANE + 1] = v2.y;
            }
        }
    } else {
        constexpr int STEP_Y = NTHR / G::IW, STEP_X = NTHR % G::IW;
        int y = threadIdx.x / G::IW, x = threadIdx.x % G::IW;
        const float* __restrict__ in0 = a.in[0];
        const float* __restrict__ in1 = a.in[1];
        const float* __restrict__ in2 = a.in[2];
        while (y < G::IH) {
            int gy = tc.iy0 + y, gx = tc.ix0 + x;
            if (GAB) {
                gy = min(max(gy, 0), H - 1);
                gx = min(max(gx, 0), W - 1);
            } else {
                gy = mirror_c(gy, H);
                gx = mirror_c(gx, W);
            }
            const uint32_t g = LAY == 1 ? plane_tiled_off(W >> 3, gy, gx) : (uint32_t)(gy * W + gx);
            const float v0 = in0[g], v1 = in1[g], v2 = in2[g];
            float* d = A + y * G::SW + x;
            d[0] = v0;
            d[G::PLANE] = v1;
            d[2 * G::PLANE] = v2;
            x += STEP_X;
            y += STEP_Y;
            if (x >= G::IW) {
                x -= G::IW;
                y++;
            }
        }
    }
    __syncthreads();
    float* cur = A;
    int m = 0;
    if (GAB) {  // Frame.performGabConvolution (:505-542). Lane = column (consecutive lanes = consecutive x: conflict-free
                // LDS rows), walking down a segment of rows with the 3x3 neighbourhood sliding through registers: three
                // new samples and 10 flops per output. (W + E) of a row is the first partial sum of both its own `adj`
                // and of the `diag` of the row below -- same operands, same order -- so it is formed once.
        m = 1;
        constexpr int rw = G::IW - 2, rh = G::IH - 2;
        constexpr int NCOLSEG = NTHR / rw;                         // row segments worked on at once
        constexpr int SEG = (rh + NCOLSEG - 1) / NCOLSEG;          // rows per segment
        constexpr int NSEG = (rh + SEG - 1) / SEG;
        static_assert(NSEG * rw <= NTHR, "one pass");
        const int seg = threadIdx.x / rw, x = threadIdx.x - seg * rw;
        const int y0 = seg * SEG;
        float go[3][SEG];
        if (seg < NSEG) {
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const float* p = cur + c * G::PLANE + y0 * G::SW + x;
                float a0 = p[0], a1 = p[1], a2 = p[2];
                float b0 = p[G::SW], b1 = p[G::SW + 1], b2 = p[G::SW + 2];
                float hs_a = a0 + a2;
                const float wb = a.p.gab_base[c], wa = a.p.gab_adj[c], wd = a.p.gab_diag[c];
#pragma unroll
                for (int k = 0; k < SEG; k++) {
                    if (y0 + k < rh) {
                        const float c0 = p[(k + 2) * G::SW], c1 = p[(k + 2) * G::SW + 1], c2 = p[(k + 2) * G::SW + 2];
                        const float hs_b = b0 + b2;
                        const float adj = hs_b + a1 + c1;    // p[-1] + p[1] + p[-SW] + p[SW]
                        const float diag = hs_a + c0 + c2;   // p[-SW-1] + p[-SW+1] + p[SW-1] + p[SW+1]
                        go[c][k] = wb * b1 + wa * adj + wd * diag;
                        a1 = b1;
                        hs_a = hs_b;
                        b0 = c0; b1 = c1; b2 = c2;
                    }
                }
            }
        }
        __syncthreads();  // every read of the un-filtered tile is done: write the results over it
        if (seg < NSEG) {
#pragma unroll
            for (int c = 0; c < 3; c++) {
                float* o = cur + c * G::PLANE + (y0 + 1) * G::SW + x + 1;
#pragma unroll
                for (int k = 0; k < SEG; k++)
                    if (y0 + k < rh) o[k * G::SW] = go[c][k];
            }
        }
        if (tc.edge && ITERS > 0) mirror_fixup<G, NTHR>(cur, m, G::RE, tc);
        __syncthreads();
    }

    // interior and edge tiles part here, at one workgroup-uniform branch: the interior path carries no coordinate clamp, no mirror
    // fix-up and no frame-bound test in its sink
    // (float planes only: the quantising sinks keep the one general path -- a second copy of their transfer code costs them registers)
    if (SK != SK_PLAIN || tc.edge) restore_epf_stages<GAB, ITERS, SK, PH, true, PLAINDIV>(a, cur, m, tc, sig, scy0, scx0);
    else restore_epf_stages<GAB, ITERS, SK, PH, false, PLAINDIV>(a, cur, m, tc, sig, scy0, scx0);
}

// the EPF iterations and the sink of one tile (after Gaborish): m = margin of the current region inside the input tile
template <bool GAB, int ITERS, int SK, int PH, bool EDGE, bool PLAINDIV>
__device__ __forceinline__ void restore_epf_stages(const FusedArgs& a, float* cur, int m, const TileCtx& tc, const float* __restrict__ sig,
                                                   int scy0, int scx0) {
    using G = Geo<GAB, ITERS>;
    constexpr int NTHR = 512 / PH;
    // final sink: XYB + transfer/quantise + global store
    const OutSink<SK, (ITERS != 4), EDGE> sink{a, tc};  // (ITERS == 4: the first half of a two-launch run -- its planes are read again at once)

    if (ITERS == 0) {
        const int mm = m;
        for (int i = threadIdx.x; i < G::OW * G::OH; i += NTHR) {
            const int y = mm + i / G::OW, x = mm + i % G::OW;
            sink(y, x, cur[y * G::SW + x], cur[G::PLANE + y * G::SW + x], cur[2 * G::PLANE + y * G::SW + x]);
        }
        return;
    }
    if (ITERS == 4) {  // iteration 0 on the whole 64x32 window, straight to the sink
        m += 3;
        epf_stage<0, G, true, PH, EDGE, PLAINDIV>(cur, m, tc, sig, scy0, scx0, a.p.epf[0], sink);
        return;
    }
    if (ITERS == 3) {
        m += 3;
        epf_stage<0, G, false, PH, EDGE, PLAINDIV>(cur, m, tc, sig, scy0, scx0, a.p.epf[0], sink);
        if (EDGE) mirror_fixup<G, NTHR>(cur, m, G::R1 + G::R2, tc);
        __syncthreads();
    }
    m += 2;
    if (ITERS >= 2) {
        epf_stage<1, G, false, PH, EDGE, PLAINDIV>(cur, m, tc, sig, scy0, scx0, a.p.epf[1], sink);
        if (EDGE) mirror_fixup<G, NTHR>(cur, m, G::R2, tc);
        __syncthreads();
        m += 1;
        epf_stage<2, G, true, PH, EDGE, PLAINDIV>(cur, m, tc, sig, scy0, scx0, a.p.epf[2], sink);
    } else {
        epf_stage<1, G, true, PH, EDGE, PLAINDIV>(cur, m, tc, sig, scy0, scx0, a.p.epf[1], sink);
    }
}

#define JXL_RESTORE_BOUNDS(ITERS, PH) __launch_bounds__(512 / PH, ITERS >= 3 ? (PH == 1 ? 4 : JXL_EPF3_PH2_WAVES) : PH == 1 ? 8 : 4)
// occupancy floor: 8 waves per SIMD (64 VGPRs); the 3-iteration variant holds 48 tap distances per patch and spilled 130
// VGPRs at that bound, so it is allowed 128 registers (4 waves per SIMD; its 43 KB tile allows 3 workgroups per CU anyway)
// PLAINDIV: the EPF tails with plain divisions (epf_patch), for the parameter sets epf_weights_plain() names
template <bool GAB, int ITERS, int SK, int PH, int LAY = 0, bool PLAINDIV = false>
__global__ JXL_RESTORE_BOUNDS(ITERS, PH) void k_restore_fused(const FusedArgs a) {
    restore_fused_body<GAB, ITERS, SK, PH, LAY, PLAINDIV>(a);
}

// a batch of frames in one launch (jxl_vardct_run_batch): blockIdx.y = frame, argument blocks in device memory read
// through the constant address space (uniform scalar loads, as from the kernel-argument segment)
template <bool GAB, int ITERS, int SK, bool PLAINDIV = false>
__global__ JXL_RESTORE_BOUNDS(ITERS, 1) void k_restore_fused_batch(const FusedArgs* __restrict__ args) {
    typedef const __attribute__((address_space(4))) FusedArgs* cargs;
    restore_fused_body<GAB, ITERS, SK, 1, 0, PLAINDIV>(*(const FusedArgs*)((cargs)args + blockIdx.y));
}

template <bool GAB, int ITERS, int SK, int PH, int LAY = 0, bool PLAINDIV = false>
void launch_tph(const FusedArgs& a, hipStream_t s) {
    using G = Geo<GAB, ITERS>;
    if constexpr (ITERS > 0 && !PLAINDIV) {  // a negative factor in the weights: the instantiation that keeps `/`
        if (epf_weights_plain(a.p)) return launch_tph<GAB, ITERS, SK, PH, LAY, true>(a, s);
    }
    // experiment knob: extra dynamic LDS per workgroup caps the workgroups per CU (160 KiB / size), leaving wave slots to
    // the latency-bound IDCT kernels of other frames in a batch
    static const size_t pad = getenv("JXL_RESTORE_LDS_PAD") ? (size_t)atoi(getenv("JXL_RESTORE_LDS_PAD")) : 0;
    static bool attr_set = false;
    if (!attr_set) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_restore_fused<GAB, ITERS, SK, PH, LAY, PLAINDIV>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)(G::LDS_BYTES + pad));
        attr_set = true;
    }
    const int tiles_x = (a.W + G::OW - 1) / G::OW, tiles_y = (a.H + G::OH - 1) / G::OH;
    const int n_tiles = tiles_x * tiles_y;
    const dim3 grid(((n_tiles + 7) / 8) * 8);
    // stage timing (jxl_vardct_enable_stage_timing): the KERNEL's own start and stop -- what rocprofv3 reports for it -- besides the
    // stage's events on the stream, which also hold the boundary to the launch in front (r6)
    if (g_restore_kernel_ev[0] && g_restore_kernel_ev[1])
        hipExtLaunchKernelGGL((k_restore_fused<GAB, ITERS, SK, PH, LAY, PLAINDIV>), grid, dim3(512 / PH), (uint32_t)(G::LDS_BYTES + pad), s, g_restore_kernel_ev[0],
                              g_restore_kernel_ev[1], 0u, a);
    else
        hipLaunchKernelGGL((k_restore_fused<GAB, ITERS, SK, PH, LAY, PLAINDIV>), grid, dim3(512 / PH), G::LDS_BYTES + pad, s, a);
}

template <bool GAB, int ITERS, int SK, bool PLAINDIV = false>
void launch_batch_t(const FusedArgs* host_args, const FusedArgs* dev_args, int n, hipStream_t s) {
    using G = Geo<GAB, ITERS>;
    if constexpr (ITERS > 0 && !PLAINDIV) {  // (the frames of a batch are of one variant, restore_fused_variant: frame 0 speaks for all)
        if (epf_weights_plain(host_args[0].p)) return launch_batch_t<GAB, ITERS, SK, true>(host_args, dev_args, n, s);
    }
    static bool attr_set = false;
    if (!attr_set) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_restore_fused_batch<GAB, ITERS, SK, PLAINDIV>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)G::LDS_BYTES);
        attr_set = true;
    }
    int max_tiles = 0;
    for (int i = 0; i < n; i++)
        max_tiles = std::max(max_tiles, ((host_args[i].W + G::OW - 1) / G::OW) * ((host_args[i].H + G::OH - 1) / G::OH));
    const dim3 grid(((max_tiles + 7) / 8) * 8, n);
    hipLaunchKernelGGL((k_restore_fused_batch<GAB, ITERS, SK, PLAINDIV>), grid, dim3(512), G::LDS_BYTES, s, dev_args);
}

// one sink kind, every (Gaborish, EPF iterations) combination, 4x1 patches
template <int SK>
void launch_fused_sk(const FusedArgs& a, hipStream_t s) {
    const int it = a.p.epf_iters;
    if (a.tiled) {  // cell-tiled input planes (run_frame's pooled planes): the variants restore_fused_takes_tiled() names, 4x1 patches
        if (a.p.gab) {
            if (it == 0) launch_tph<true, 0, SK, 1, 1>(a, s);
            else if (it == 1) launch_tph<true, 1, SK, 1, 1>(a, s);
            else launch_tph<true, 2, SK, 1, 1>(a, s);
        } else {
            if (it == 0) launch_tph<false, 0, SK, 1, 1>(a, s);
            else if (it == 1) launch_tph<false, 1, SK, 1, 1>(a, s);
            else launch_tph<false, 2, SK, 1, 1>(a, s);
        }
        return;
    }
    if (a.p.gab) {
        if (it == 0) launch_tph<true, 0, SK, 1>(a, s);
        else if (it == 1) launch_tph<true, 1, SK, 1>(a, s);
        else if (it == 2) launch_tph<true, 2, SK, 1>(a, s);
        else if (it == 4) {
            if constexpr (SK == SK_PLAIN) launch_tph<true, 4, SK_PLAIN, 1>(a, s);  // (float planes only: the first half of a split run)
        } else launch_tph<true, 3, SK, 1>(a, s);
    } else {
        if (it == 0) launch_tph<false, 0, SK, 1>(a, s);
        else if (it == 1) launch_tph<false, 1, SK, 1>(a, s);
        else if (it == 2) launch_tph<false, 2, SK, 1>(a, s);
        else if (it == 4) {
            if constexpr (SK == SK_PLAIN) launch_tph<false, 4, SK_PLAIN, 1>(a, s);
        } else launch_tph<false, 3, SK, 1>(a, s);
    }
}
template <int SK>
void launch_fused_batch_sk(const FusedArgs* h, const FusedArgs* d, int n, hipStream_t s) {
    const int it = h[0].p.epf_iters;
    if (h[0].p.gab) {
        if (it == 0) launch_batch_t<true, 0, SK>(h, d, n, s);
        else if (it == 1) launch_batch_t<true, 1, SK>(h, d, n, s);
        else if (it == 2) launch_batch_t<true, 2, SK>(h, d, n, s);
        else launch_batch_t<true, 3, SK>(h, d, n, s);
    } else {
        if (it == 0) launch_batch_t<false, 0, SK>(h, d, n, s);
        else if (it == 1) launch_batch_t<false, 1, SK>(h, d, n, s);
        else if (it == 2) launch_batch_t<false, 2, SK>(h, d, n, s);
        else launch_batch_t<false, 3, SK>(h, d, n, s);
    }
}

}  // namespace
}  // namespace jxl
