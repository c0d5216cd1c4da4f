// N images resampled into one batch tensor in one launch: tensor_resize_body.h's resize_tile over a work list that spans the
// images. The descriptors (one ResizeArgs per image, its t.out already the image's place in the batch), the work list and the
// tap tables live in device memory -- the kernel's argument block is three pointers, whatever N is.
//
//   k_tensor_resize_batch<BYTES, COLORS>, workgroups of 256 lanes grid-striding over the global tile index g in
//   [0, tile_base[n]): the image is the i with tile_base[i] <= g < tile_base[i + 1] (a binary search over scalar loads: g is
//   the workgroup's, so every load and branch of the search is wave-uniform), its tile is g - tile_base[i], and the tile runs
//   with items[i] read through the const __restrict__ pointer where the body needs a field.
//   Neighbouring tiles of a workgroup may belong to images that differ in tile shape, LDS layout, plane count, alpha and source
//   pitch: the body takes all of these from the descriptor, per tile, and ends behind a barrier.
// Every image has at least one tile (oh, ow >= 1), so tile_base is strictly increasing and the search has one answer.
// The bytes of image i are those of k_tensor_resize launched with items[i]: the same body, and no sum crosses a lane.
#include "tensor_resize_body.h"

namespace jxl {
namespace {

template <int BYTES, int COLORS>
__global__ __launch_bounds__(256) void k_tensor_resize_batch(const ResizeArgs* __restrict__ items, const int64_t* __restrict__ tile_base,
                                                             const int32_t* __restrict__ counts) {
    extern __shared__ float lds[];
    const int n = counts[0];  // images
    const int64_t total = tile_base[n];
    for (int64_t g = blockIdx.x; g < total; g += gridDim.x) {
        int lo = 0, hi = n;  // tile_base[lo] <= g < tile_base[hi]
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (tile_base[mid] <= g) lo = mid;
            else hi = mid;
        }
        resize_tile<BYTES, COLORS>(items[lo], g - tile_base[lo], lds);
    }
}

template <int BYTES>
void launch_batch(const ResizeArgs* items, const int64_t* tile_base, const int32_t* counts, int n_color, unsigned grid, size_t lds,
                  hipStream_t s) {
    if (n_color == 3) hipLaunchKernelGGL((k_tensor_resize_batch<BYTES, 3>), dim3(grid), dim3(256), lds, s, items, tile_base, counts);
    else hipLaunchKernelGGL((k_tensor_resize_batch<BYTES, 1>), dim3(grid), dim3(256), lds, s, items, tile_base, counts);
}

}  // namespace

void launch_tensor_resize_batch(const ResizeArgs* items, const int64_t* tile_base, const int32_t* counts, int dtype, int n_color,
                                unsigned grid, int lds_bytes, hipStream_t s) {
    if (!grid) return;
    if (dtype == JXL_TENSOR_U8) launch_batch<1>(items, tile_base, counts, n_color, grid, (size_t)lds_bytes, s);
    else if (dtype == JXL_TENSOR_F32) launch_batch<4>(items, tile_base, counts, n_color, grid, (size_t)lds_bytes, s);
    else launch_batch<2>(items, tile_base, counts, n_color, grid, (size_t)lds_bytes, s);
}

}  // namespace jxl
