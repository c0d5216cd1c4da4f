// The cell-tiled layout of the pooled IDCT-output planes: a plane of H x W samples (both multiples of 8) as
// (H / 8) x (W / 8) cells of 64 consecutive floats (256 bytes = two 128-byte lines), row-major 8x8 inside a cell:
//   off(y, x) = ((y >> 3) * (W >> 3) + (x >> 3)) * 64 + (y & 7) * 8 + (x & 7)
// -- the layout the quantised-coefficient planes have had since r4 (coeff_off). Written by the 256-thread IDCT launch
// (k_idct_wg3.hip) and read by the one fused restoration launch behind it (restore_fused_body.h); nothing else ever sees such a
// plane, so everything that has to agree on the layout is in this header. Runs of 4 (8) samples that start at a multiple of 4 (8)
// stay inside one cell row: 16- and 32-byte accesses never straddle a cell.
// Plain C++ (no HIP header): tools/native/plane_tiled_check.cpp compiles it for the host alone.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define JXL_PT_HD __host__ __device__ __forceinline__
#else
#define JXL_PT_HD inline
#endif

namespace jxl {

// sample offsets are formed in 32 bits off the plane base (the restoration kernel has always done so for raster planes)
JXL_PT_HD bool plane_tiled_ok(int W, int H) {
    return W >= 8 && H >= 8 && (W & 7) == 0 && (H & 7) == 0 && (int64_t)W * H < ((int64_t)1 << 31);
}

// cells_w = W >> 3
JXL_PT_HD uint32_t plane_tiled_off(int cells_w, int y, int x) {
    return ((uint32_t)((y >> 3) * cells_w + (x >> 3)) << 6) + (uint32_t)(((y & 7) << 3) | (x & 7));
}

}  // namespace jxl
