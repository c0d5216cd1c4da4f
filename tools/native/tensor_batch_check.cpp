// Stand-alone host check of jxlatte_amd/csrc/tensor_batch_check.h (no device, no context), meant for an AddressSanitizer +
// UBSan build (tests/test_tensor_batch_cpu.py): the refusals of the batch itself, the agreement of the items, the tensors'
// offsets in 64 bits, the sharing of tap tables, the work list with its cap, the search the kernel makes in it, the LDS maximum
// and the grid, over a table of cases. Then, for every "oh ow tw th" quadruple on the command line, one item of a work list:
//   BASE <n> <tile_base[0]> ... <tile_base[n]>
// Ends with "<n> failure(s)".
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../jxlatte_amd/csrc/tensor_batch_check.h"

static int failures = 0;
#define EXPECT(cond, what)                          \
    do {                                            \
        if (!(cond)) {                              \
            printf("FAIL: %s (%s)\n", what, #cond); \
            failures++;                             \
        }                                           \
    } while (0)

static jxl_tensor_batch_item item(int source, int h, int w, int oh, int ow) {
    jxl_tensor_batch_item it;
    memset(&it, 0, sizeof it);
    it.source = source, it.set_id = -1, it.alpha_plane = -1;
    it.p.color.n_planes = 3;
    it.p.height = h, it.p.width = w;
    it.p.dtype = JXL_TENSOR_F32, it.p.layout = JXL_TENSOR_CHW;
    it.p.alpha_tagged_depth = it.p.color_tagged_depth = 8;
    const jxl_resize_params r = {0, 0, w, h, oh, ow, JXL_RESIZE_TRIANGLE};
    it.r = r;
    return it;
}

static void refusals() {
    std::vector<jxl_tensor_batch_item> v(4, item(JXL_BATCH_HOST, 33, 67, 2, 5));
    int out = 0, bad = 7;
    EXPECT(jxl::batch_check_items(4, v.data(), &out, &bad) == nullptr && bad == -1, "four host items");
    EXPECT(jxl::batch_check_items(0, v.data(), &out, &bad) && bad == -1, "n = 0");
    EXPECT(jxl::batch_check_items(-1, v.data(), &out, &bad), "n < 0");
    EXPECT(jxl::batch_check_items(jxl::kBatchMaxItems + 1, v.data(), &out, &bad), "n above the cap (nothing of that length is read)");
    EXPECT(jxl::kBatchMaxItems >= 256, "the cap is not below 256");
    EXPECT(jxl::batch_check_items(4, nullptr, &out, &bad) && jxl::batch_check_items(4, v.data(), nullptr, &bad), "null arguments");
    v[2].source = 3;
    EXPECT(jxl::batch_check_items(4, v.data(), &out, &bad) && bad == 2, "an unknown source, by index");
    v[2].source = -1;
    EXPECT(jxl::batch_check_items(4, v.data(), &out, &bad) && bad == 2, "a negative source");
    v[2].source = JXL_BATCH_SET;
    v[1].source = JXL_BATCH_RESIDENT;
    EXPECT(jxl::batch_check_items(4, v.data(), &out, &bad) == nullptr, "a set, the resident planes and host arrays in one batch");
    v[3].source = JXL_BATCH_RESIDENT;
    EXPECT(jxl::batch_check_items(4, v.data(), &out, &bad) && bad == 3, "a second resident item, by index");
    v[3].source = JXL_BATCH_SET, v[3].set_id = v[2].set_id = 5;
    EXPECT(jxl::batch_check_items(4, v.data(), &out, &bad) == nullptr, "two items may name one set");
}

static void agreement() {
    const jxl_tensor_batch_item a = item(JXL_BATCH_HOST, 33, 67, 2, 5);
    jxl::TensorLayout la, lb;
    jxl_tensor_params q = a.p;
    q.height = 2, q.width = 5;
    EXPECT(jxl::tensor_check_params(&q, &la) == nullptr, "the first item's layout");
    const jxl::BatchShape first = jxl::batch_shape(a.p, a.r, la);
    jxl_tensor_batch_item b = item(JXL_BATCH_HOST, 5, 7, 2, 5);
    b.r.filter = JXL_RESIZE_BOX, b.p.use_norm = 1, b.p.color.tf_in = 2;
    EXPECT(jxl::batch_check_agree(first, jxl::batch_shape(b.p, b.r, la)) == nullptr, "source size, filter, colour, normalisation are per item");
    b.r.out_height = 3;
    EXPECT(jxl::batch_check_agree(first, jxl::batch_shape(b.p, b.r, la)), "another output height");
    b.r.out_height = 2, b.r.out_width = 4;
    EXPECT(jxl::batch_check_agree(first, jxl::batch_shape(b.p, b.r, la)), "another output width");
    b.r.out_width = 5, b.p.dtype = JXL_TENSOR_F16;
    EXPECT(jxl::batch_check_agree(first, jxl::batch_shape(b.p, b.r, la)), "another dtype");
    b.p.dtype = JXL_TENSOR_F32, b.p.layout = JXL_TENSOR_HWC;
    EXPECT(jxl::batch_check_agree(first, jxl::batch_shape(b.p, b.r, la)), "another layout");
    b.p.layout = JXL_TENSOR_CHW, b.p.color.n_planes = 1;  // a grey image among colour ones
    q = b.p, q.height = 2, q.width = 5;
    EXPECT(jxl::tensor_check_params(&q, &lb) == nullptr && lb.n_out == 1, "a grey item's layout");
    EXPECT(jxl::batch_check_agree(first, jxl::batch_shape(b.p, b.r, lb)), "another channel count");
    b.p.color.n_planes = 3, b.p.has_alpha = b.p.write_alpha = 1;
    q = b.p, q.height = 2, q.width = 5;
    EXPECT(jxl::tensor_check_params(&q, &lb) == nullptr && lb.n_out == 4, "alpha written");
    EXPECT(jxl::batch_check_agree(first, jxl::batch_shape(b.p, b.r, lb)), "alpha written on one item only");
    b.p.write_alpha = 0, b.p.premultiplied = 1;
    q = b.p, q.height = 2, q.width = 5;
    EXPECT(jxl::tensor_check_params(&q, &lb) == nullptr && jxl::batch_check_agree(first, jxl::batch_shape(b.p, b.r, lb)) == nullptr,
           "alpha read but dropped beside an item without alpha");
}

static void offsets() {
    std::vector<uint64_t> off;
    uint64_t total = 0;
    EXPECT(jxl::batch_offsets(3, 120, &off, &total) == nullptr && off.size() == 3 && off[0] == 0 && off[1] == 120 && off[2] == 240 && total == 360, "three tensors");
    EXPECT(jxl::batch_offsets(1, 1, &off, &total) == nullptr && off.size() == 1 && off[0] == 0 && total == 1, "a batch of one");
    const uint64_t big = (uint64_t)3 << 31;  // a tensor past 2^32 bytes: the offsets need 64 bits
    EXPECT(jxl::batch_offsets(1024, big, &off, &total) == nullptr && off[1023] == 1023 * big && total == 1024 * big && off[2] > UINT32_MAX, "offsets in 64 bits");
    EXPECT(jxl::batch_offsets(1024, (uint64_t)1 << 53, &off, &total), "a batch past 63 bits");
    EXPECT(jxl::batch_offsets(2, (uint64_t)INT64_MAX, &off, &total), "two tensors of 2^63 - 1 bytes");
    EXPECT(jxl::batch_offsets(0, 120, &off, &total) && jxl::batch_offsets(3, 0, &off, &total), "no items, no bytes");
}

static void sharing() {
    jxl::BatchTableSet set;
    const char* why = nullptr;
    // two items of 33 x 67 -> 2 x 5, one of them boxed to 9 x 20, one 5 x 7 with the other filter
    const int y0 = set.find(0, 33, 2, JXL_RESIZE_TRIANGLE, &why), x0 = set.find(1, 67, 5, JXL_RESIZE_TRIANGLE, &why);
    const int y1 = set.find(0, 33, 2, JXL_RESIZE_TRIANGLE, &why), x1 = set.find(1, 67, 5, JXL_RESIZE_TRIANGLE, &why);
    EXPECT(y0 >= 0 && x0 >= 0 && y0 != x0 && y1 == y0 && x1 == x0 && set.tables.size() == 2, "the same source and output length share a table");
    const int yb = set.find(0, 9, 2, JXL_RESIZE_TRIANGLE, &why), xb = set.find(1, 20, 5, JXL_RESIZE_TRIANGLE, &why);
    EXPECT(yb >= 0 && xb >= 0 && yb != y0 && xb != x0 && set.tables.size() == 4, "a boxed item of another length does not");
    const int yf = set.find(0, 33, 2, JXL_RESIZE_BOX, &why);
    EXPECT(yf >= 0 && yf != y0 && set.tables.size() == 5, "another filter does not");
    const int ya = set.find(1, 33, 2, JXL_RESIZE_TRIANGLE, &why);
    EXPECT(ya >= 0 && ya != y0 && set.tables.size() == 6, "tables are per axis");
    EXPECT(set.asked == 8 && set.asked - (int)set.tables.size() == 2, "lookups and tables built");
    EXPECT(set.tables[(size_t)y0].first.size() == 2 && set.tables[(size_t)x0].first.size() == 5 && set.tables[(size_t)xb].first.size() == 5, "the tables' lengths");
    EXPECT(set.find(1, 2100, 1, JXL_RESIZE_TRIANGLE, &why) == -1 && why && strstr(why, "1024 taps") && set.tables.size() == 6, "a refused table is not kept");
    EXPECT(set.find(0, 33, 2, JXL_RESIZE_TRIANGLE, &why) == y0, "earlier indices stay");
}

static void worklist() {
    std::vector<int64_t> base;
    EXPECT(jxl::batch_item_tiles(2, 5, 8, 2) == 1 && jxl::batch_item_tiles(13, 11, 8, 4) == 8 && jxl::batch_item_tiles(1, 1, 64, 4) == 1 &&
               jxl::batch_item_tiles(224, 224, 32, 4) == 392,
           "tiles of an item");
    EXPECT(jxl::batch_tile_base({1, 8, 1, 392}, &base) == nullptr && base.size() == 5 && base[0] == 0 && base[1] == 1 && base[2] == 9 && base[3] == 10 && base[4] == 402,
           "the prefix sum");
    bool found = true;
    for (int64_t g = 0; g < base[4]; g++) {
        const int i = jxl::batch_find_item(base, g);
        found = found && base[(size_t)i] <= g && g < base[(size_t)i + 1];
    }
    EXPECT(found && jxl::batch_find_item(base, 0) == 0 && jxl::batch_find_item(base, 1) == 1 && jxl::batch_find_item(base, 9) == 2 && jxl::batch_find_item(base, 10) == 3 &&
               jxl::batch_find_item(base, 401) == 3,
           "the search: single-tile items between larger ones");
    EXPECT(jxl::batch_tile_base({5}, &base) == nullptr && base.size() == 2 && base[1] == 5 && jxl::batch_find_item(base, 4) == 0, "a batch of one");
    std::vector<int64_t> ones(1024, 1);
    EXPECT(jxl::batch_tile_base(ones, &base) == nullptr && base[1024] == 1024 && jxl::batch_find_item(base, 777) == 777, "1024 single-tile items");
    EXPECT(jxl::batch_tile_base({3, 0, 2}, &base) && jxl::batch_tile_base({-1}, &base), "an item without tiles");
    EXPECT(jxl::batch_tile_base({jxl::kBatchMaxTiles}, &base) == nullptr && base[1] == jxl::kBatchMaxTiles, "the cap itself");
    EXPECT(jxl::batch_tile_base({jxl::kBatchMaxTiles, 1}, &base), "one tile past the cap");
    EXPECT(jxl::batch_tile_base({INT64_MAX, INT64_MAX}, &base), "counts that would wrap 63 bits");
    EXPECT(jxl::batch_lds_bytes({512, 65536, 4}) == 65536 && jxl::batch_lds_bytes({16}) == 16 && jxl::batch_lds_bytes({}) == 0, "the LDS maximum");
    EXPECT(jxl::batch_grid(402, 65536) == 402 && jxl::batch_grid(402, 3) == 3 && jxl::batch_grid(402, 1) == 1 && jxl::batch_grid(402, 0) == 1 &&
               jxl::batch_grid(jxl::kBatchMaxTiles, 65536) == 65536,
           "the grid");
}

int main(int argc, char** argv) {
    refusals();
    agreement();
    offsets();
    sharing();
    worklist();
    std::vector<int64_t> tiles;
    for (int i = 1; i + 3 < argc; i += 4)
        tiles.push_back(jxl::batch_item_tiles(atol(argv[i]), atol(argv[i + 1]), atoi(argv[i + 2]), atoi(argv[i + 3])));
    if (!tiles.empty()) {
        std::vector<int64_t> base;
        const char* why = jxl::batch_tile_base(tiles, &base);
        if (why) printf("BASE refused: %s\n", why);
        else {
            printf("BASE %zu", tiles.size());
            for (int64_t b : base) printf(" %" PRId64, b);
            printf("\n");
        }
    }
    printf("%d failure(s)\n", failures);
    return failures ? 1 : 0;
}
