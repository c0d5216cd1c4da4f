// Frame.synthesizeNoise's arithmetic for one pixel (Frame.java:790-831) and the tap weight of initializeNoise's 5x5 high-pass
// (Frame.java:57-63), stated once: k_post.hip (k_noise_add, whole planes) and k_noise_window.hip (a window of a frame) call them.
// Every expression keeps the reference's association (the files that include this are compiled with -ffp-contract=off).
#pragma once
#include <hip/hip_runtime.h>

#include "sample_ops.h"

namespace jxl {

// 0.16 everywhere, -3.84 at the centre
__device__ __forceinline__ float noise_tap(int iy, int ix) { return (iy == 2 && ix == 2) ? -3.84f : 0.16f; }

// lut: the frame's eight noise parameters; n0..n2: the three convolved noise channels at the pixel; X, Y, B are updated
__device__ __forceinline__ void noise_add_px(const float* lut, float n0, float n1, float n2, float bcx, float bcb, float& X, float& Y, float& B) {
    const float bx = X, by = Y, bb = B;
    float inR = by + bx;
    inR = inR < 0.0f ? 0.0f : 3.0f * inR;
    float inG = by - bx;
    inG = inG < 0.0f ? 0.0f : 3.0f * inG;
    int iR, iG;
    float fR, fG;
    if (inR >= 7.0f) { iR = 6; fR = 1.0f; } else { iR = java_f2i(inR); fR = inR - (float)iR; }
    if (inG >= 7.0f) { iG = 6; fG = 1.0f; } else { iG = java_f2i(inG); fG = inG - (float)iG; }
    float sr = (lut[iR + 1] - lut[iR]) * fR + lut[iR];
    float sg = (lut[iG + 1] - lut[iG]) * fG + lut[iG];
    sr = sr < 0.0f ? 0.0f : sr > 1.0f ? 1.0f : sr;
    sg = sg < 0.0f ? 0.0f : sg > 1.0f ? 1.0f : sg;
    const float nr = sr * (0.00171875f * n0 + 0.21828125f * n2);
    const float ng = sg * (0.00171875f * n1 + 0.21828125f * n2);
    const float nrg = nr + ng;
    Y = by + nrg;
    X = bx + (bcx * nrg + nr - ng);
    B = bb + bcb * nrg;
}

}  // namespace jxl
