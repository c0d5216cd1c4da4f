// The three quotients of an EPF pixel -- sumChannels[c] / sumWeights, c = 0..2 (Frame.java:627-629) -- with the denominator's half
// of the division formed once. Bit-identical to three `n / d` of the compiler by construction; restore_fused_body.h is the user,
// jxl_debug_epf_quot3 (host.hip) runs it on arrays for tests/test_epf_quot3_gpu.py.
//
// What `n / d` is on gfx950 (f32, correctly rounded, denormals kept -- the library's flags):
//     ds = v_div_scale(d, d, n)   ns = v_div_scale(n, d, n)            (VCC = "the pair was scaled")
//     r0 = v_rcp(ds)              e0 = fma(-ds, r0, 1)                 r1 = fma(e0, r0, r0)
//     q0 = ns * r1                e1 = fma(-ds, q0, ns)                q1 = fma(e1, r1, q0)
//     e2 = fma(-ds, q1, ns)       q  = v_div_fmas(e2, r1, q1)          result = v_div_fixup(q, d, n)
// v_div_scale returns its first operand unchanged and leaves VCC clear unless one of these holds (the ISA's list, E = biased exponent):
//     n == 0 or d == 0;   E(n) - E(d) >= 96;   d denormal;   1 / d denormal;   n / d denormal;   E(n) <= 23.
// v_div_fmas with VCC clear is fma(e2, r1, q1). v_div_fixup returns |q| with the sign of n ^ d unless n or d is NaN, infinite or
// zero, or E(n) - E(d) < -150, or E(d) == 255.
//
// The window. d is a sum of weights, 1 <= d < 16 (E(d) in 127..130; see restore_fused_body.h for why that holds for every pixel, the
// skipped ones included). For such a d none of the cases above can occur when every numerator satisfies
//     2^-100 <= |n| <= 2^90        (E(n) in 27..217:  E(n) > 23,  E(n) - E(d) in -103..90,  |n / d| > 2^-104, nothing is zero,
//                                   infinite or NaN, and q has the sign of n because d > 0)
// so both v_div_scale are moves, v_div_fmas is an fma and v_div_fixup a move: what remains is the sequence of epf_quot_refined_rcp /
// epf_quot_by below on the same operands in the same order. r0, e0, r1 do not depend on the numerator: formed once per pixel.
// The window is tested, not assumed: the smallest magnitude against 2^-100 and the SUM of the magnitudes against 2^90 (a sum of
// non-negative floats is at least each of them, and unlike v_max3 it does not drop a NaN: NaN and infinity fail the test). If any
// lane of the wave fails for any pixel of its patch, the whole wave takes the plain divisions for that patch -- a wave-uniform
// branch. Zeros of either sign, denormals, huge samples, infinities and NaNs therefore go through `n / d` as before.
#pragma once
#include <hip/hip_runtime.h>

namespace jxl {

constexpr float kEpfQuotLo = 0x1p-100f;  // smallest numerator magnitude of the fast path
constexpr float kEpfQuotHi = 0x1p+90f;   // bound on the sum of the magnitudes tested together (so on each of them)

// every numerator of an NP-pixel patch inside the window: the smallest magnitude and the sum of all of them, two compares
template <int NP>
__device__ __forceinline__ bool epf_quot3_in_window(const float n[3][NP]) {
    float lo = __builtin_fabsf(n[0][0]), sum = lo;
#pragma unroll
    for (int k = 1; k < 3 * NP; k++) {
        const float a = __builtin_fabsf(n[k % 3][k / 3]);
        lo = __builtin_fminf(lo, a);
        sum = sum + a;
    }
    return lo >= kEpfQuotLo && sum <= kEpfQuotHi;
}

// the numerator-independent half of n / d, for 1 <= d < 16
__device__ __forceinline__ float epf_quot_refined_rcp(float d) {
    const float r0 = __builtin_amdgcn_rcpf(d);
    const float e0 = __builtin_fmaf(-d, r0, 1.0f);
    return __builtin_fmaf(e0, r0, r0);
}
// n / d from r1 = epf_quot_refined_rcp(d), for n inside the window
__device__ __forceinline__ float epf_quot_by(float n, float d, float r1) {
    const float q0 = n * r1;
    const float e1 = __builtin_fmaf(-d, q0, n);
    const float q1 = __builtin_fmaf(e1, r1, q0);
    const float e2 = __builtin_fmaf(-d, q1, n);
    return __builtin_fmaf(e2, r1, q1);
}

// out[c][i] = n[c][i] / d[i], bit for bit, for the NP pixels of a register patch: 1 <= d[i] < 16, ANY numerators. ONE test and one
// wave-uniform branch per patch (a branch per pixel pinned the register allocation of the fused kernel's 64-register variants into
// scratch): every numerator of the patch inside the window -> the shared-reciprocal sequence for all of them, else the plain
// divisions for all of them.
// plain(c, i, q): what the plain-division branch -- and only that branch -- stores for quotient q of channel c, pixel i. The fused
// kernel keeps its select of skipped pixels there (restore_fused_body.h, epf_patch, says why the fast branch needs none).
template <int NP, typename Plain>
__device__ __forceinline__ void epf_quot3_patch(const float n[3][NP], const float d[NP], float out[3][NP], Plain plain) {
    if (__builtin_expect(__builtin_amdgcn_ballot_w64(!epf_quot3_in_window<NP>(n)) == 0, 1)) {
#pragma unroll
        for (int i = 0; i < NP; i++) {
            const float r1 = epf_quot_refined_rcp(d[i]);
#pragma unroll
            for (int c = 0; c < 3; c++) out[c][i] = epf_quot_by(n[c][i], d[i], r1);
        }
    } else {
#pragma unroll
        for (int i = 0; i < NP; i++)
#pragma unroll
            for (int c = 0; c < 3; c++) out[c][i] = plain(c, i, n[c][i] / d[i]);
    }
}
template <int NP>
__device__ __forceinline__ void epf_quot3_patch(const float n[3][NP], const float d[NP], float out[3][NP]) {
    epf_quot3_patch<NP>(n, d, out, [](int, int, float q) { return q; });
}

// one pixel: out[c] = nc / d (the patch form with NP = 1; what jxl_debug_epf_quot3 runs, one lane per element)
__device__ __forceinline__ void epf_quot3(float n0, float n1, float n2, float d, float out[3]) {
    const float n[3][1] = {{n0}, {n1}, {n2}}, dd[1] = {d};
    float q[3][1];
    epf_quot3_patch<1>(n, dd, q);
    out[0] = q[0][0];
    out[1] = q[1][0];
    out[2] = q[2][0];
}

}  // namespace jxl
