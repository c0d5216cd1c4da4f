// The pure part of the batched resized tensor entry (tensor_batch_host.hip): the refusals of the batch itself, the sharing of
// tap tables inside a call, the work list, the launch's LDS size and each image's place in the batch tensor. Plain C++: no device
// call, no context; tools/native/tensor_batch_check.cpp runs it as a program of its own under the sanitizers. Everything about
// ONE image -- its parameters, box, tables, tile -- is tensor_check.h's and tensor_resize_check.h's, asked per item.
#ifndef JXL_TENSOR_BATCH_CHECK_H
#define JXL_TENSOR_BATCH_CHECK_H
#include <map>
#include <stdint.h>
#include <tuple>
#include <vector>

#include "tensor_resize_check.h"

namespace jxl {

constexpr int kBatchMaxItems = JXL_TENSOR_BATCH_MAX;
// the work list's total: far above any batch whose tensors fit a device's memory (a tile writes at least one element), and low
// enough that no sum of kBatchMaxItems tile counts, each checked against it, comes near 63 bits
constexpr int64_t kBatchMaxTiles = (int64_t)1 << 40;

// nullptr, or why the batch's own arguments are refused, before any item is looked at: n, the pointers, the source kinds, the
// one set of resident planes. *bad: the item the refusal is about, or -1
inline const char* batch_check_items(int32_t n, const jxl_tensor_batch_item* items, const void* out, int* bad) {
    *bad = -1;
    if (n < 1 || n > kBatchMaxItems) return "tensor batch: the item count is out of range";
    if (!items || !out) return "tensor batch: null argument";
    int resident = 0;
    for (int i = 0; i < n; i++) {
        const int32_t s = items[i].source;
        if (s != JXL_BATCH_HOST && s != JXL_BATCH_RESIDENT && s != JXL_BATCH_SET) return *bad = i, "tensor batch: unknown source";
        if (s == JXL_BATCH_RESIDENT && ++resident > 1) return *bad = i, "tensor batch: a context has one set of resident planes";
    }
    return nullptr;
}

// what every item of a batch shares, taken from an item's parameters and the layout tensor_check_params gave it
struct BatchShape {
    int32_t oh, ow, dtype, layout;
    int n_out;
};
inline BatchShape batch_shape(const jxl_tensor_params& p, const jxl_resize_params& r, const TensorLayout& lay) {
    return BatchShape{r.out_height, r.out_width, p.dtype, p.layout, lay.n_out};
}
// nullptr, or in what an item disagrees with the batch's first
inline const char* batch_check_agree(const BatchShape& first, const BatchShape& it) {
    if (it.oh != first.oh || it.ow != first.ow) return "tensor batch: the items disagree on the output size";
    if (it.dtype != first.dtype) return "tensor batch: the items disagree on the dtype";
    if (it.layout != first.layout) return "tensor batch: the items disagree on the layout";
    if (it.n_out != first.n_out) return "tensor batch: the items disagree on the channel count";
    return nullptr;
}

// item i's tensor starts i * bytes_each bytes into the batch, which is n * bytes_each bytes: in 64 bits, refused where the whole
// does not fit 63
inline const char* batch_offsets(int32_t n, uint64_t bytes_each, std::vector<uint64_t>* off, uint64_t* total) {
    if (n < 1 || bytes_each == 0) return "tensor batch: the item count is out of range";
    if (bytes_each > (uint64_t)INT64_MAX / (uint64_t)n) return "tensor batch: the batch's size does not fit 63 bits";
    off->resize((size_t)n);
    for (int32_t i = 0; i < n; i++) (*off)[(size_t)i] = (uint64_t)i * bytes_each;
    *total = (uint64_t)n * bytes_each;
    return nullptr;
}

// Table sharing: one table per distinct (length, output length, filter) per axis within a call. A table is relative to its box,
// so the box's origin is no part of the key.
struct BatchTableSet {
    std::map<std::tuple<int, int64_t, int64_t, int>, int> index;  // (axis, L, O, filter) -> tables[]
    std::vector<ResizeTaps> tables;
    int asked = 0;  // find() calls: asked - tables.size() were shared
    // the table's index in `tables`, built on first use; -1 and *why when resize_build_taps refuses it
    int find(int axis, int64_t L, int64_t O, int filter, const char** why) {
        asked++;
        const auto key = std::make_tuple(axis, L, O, filter);
        const auto it = index.find(key);
        if (it != index.end()) return it->second;
        ResizeTaps t;
        if ((*why = resize_build_taps(L, O, filter, &t))) return -1;
        tables.push_back(std::move(t));
        return index[key] = (int)tables.size() - 1;
    }
};

// the tiles of one item
inline int64_t batch_item_tiles(int64_t oh, int64_t ow, int tw, int th) { return ((ow + tw - 1) / tw) * ((oh + th - 1) / th); }

// The work list: tile_base[n + 1], the prefix sum of the items' tile counts. Every count is >= 1 (the kernel's search relies on a
// strictly increasing list) and the total at most kBatchMaxTiles
inline const char* batch_tile_base(const std::vector<int64_t>& tiles, std::vector<int64_t>* base) {
    base->assign(tiles.size() + 1, 0);
    for (size_t i = 0; i < tiles.size(); i++) {
        if (tiles[i] < 1) return "tensor batch: an item without tiles";
        if (tiles[i] > kBatchMaxTiles - (*base)[i]) return "tensor batch: too many tiles";
        (*base)[i + 1] = (*base)[i] + tiles[i];
    }
    return nullptr;
}

// the item of global tile g (the kernel's search, for the tool's table): tile_base[i] <= g < tile_base[i + 1]
inline int batch_find_item(const std::vector<int64_t>& base, int64_t g) {
    int lo = 0, hi = (int)base.size() - 1;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (base[(size_t)mid] <= g) lo = mid;
        else hi = mid;
    }
    return lo;
}

// the launch's dynamic LDS: the largest image of vertical sums among the items' tiles
inline int batch_lds_bytes(const std::vector<int>& lds_bytes) {
    int most = 0;
    for (int b : lds_bytes)
        if (b > most) most = b;
    return most;
}

// the grid: a workgroup per tile up to `bound` (the device's own limit, or a test's)
inline unsigned batch_grid(int64_t total, int64_t bound) {
    if (bound < 1) bound = 1;
    return (unsigned)(total < bound ? total : bound);
}

}  // namespace jxl
#endif  // JXL_TENSOR_BATCH_CHECK_H
