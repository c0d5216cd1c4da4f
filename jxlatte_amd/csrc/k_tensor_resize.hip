// The image resampled to a device tensor of a given size in one pass: k_tensor_samples with a separable filter between its
// stages 5 and 6, so that the filter works on linear samples wherever the plan has a linear intermediate and the transfer curve
// of the output (the f64 chains) is evaluated per OUTPUT pixel only.
//
//   k_tensor_resize<BYTES, COLORS>, one workgroup of 256 lanes per output tile of tw columns x th rows (th <= 4), grid-striding
//   over the tiles of ONE image whose descriptor is the kernel's argument. The tile itself -- V pass, LDS image, H pass, tail,
//   store -- is tensor_resize_body.h's resize_tile, which k_tensor_resize_batch.hip runs over a work list of many images.
#include "tensor_resize_body.h"

namespace jxl {
namespace {

template <int BYTES, int COLORS>
__global__ __launch_bounds__(256) void k_tensor_resize(const ResizeArgs r) {
    extern __shared__ float lds[];
    const int64_t tiles = resize_tiles(r);
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) resize_tile<BYTES, COLORS>(r, tile, lds);
}

template <int BYTES>
void launch_resize(const ResizeArgs& r, int n_color, unsigned grid, hipStream_t s) {
    if (n_color == 3) hipLaunchKernelGGL((k_tensor_resize<BYTES, 3>), dim3(grid), dim3(256), (size_t)r.lds_bytes, s, r);
    else hipLaunchKernelGGL((k_tensor_resize<BYTES, 1>), dim3(grid), dim3(256), (size_t)r.lds_bytes, s, r);
}

}  // namespace

void launch_tensor_resize(const ResizeArgs& r, hipStream_t s) {
    const int64_t tiles = resize_tiles(r);
    if (tiles <= 0) return;
    const unsigned grid = (unsigned)(tiles < 65536 ? tiles : 65536);
    const int n_color = (r.t.g.c.n_planes == 3 || r.t.g.c.use_matrix || r.t.g.c.use_tone_map) ? 3 : 1;
    if (r.t.dtype == JXL_TENSOR_U8) launch_resize<1>(r, n_color, grid, s);
    else if (r.t.dtype == JXL_TENSOR_F32) launch_resize<4>(r, n_color, grid, s);
    else launch_resize<2>(r, n_color, grid, s);
}

}  // namespace jxl
