// Host side of the batched resized tensor exit (k_tensor_resize_batch.hip): jxl_tensor_resized_batch. Per item it resolves the
// image's home from the item's source kind (one switch) and makes the checks of the single-image entries on it -- through the
// functions those entries call themselves (tensor_host.h), in their order -- and plans the item's launch as they do; what is
// the batch's own (its refusals, the sharing of tables, the work list, the LDS size, the tensors' places) is
// tensor_batch_check.h's. Nothing is queued before every item has passed; the descriptors, the work list and the tables go up in
// ONE transfer; one launch; the stream is synchronised once.
#include "tensor_batch_check.h"
#include "tensor_host.h"

#include <cstdio>
#include <cstring>
#include <string>

namespace jxl {
namespace {

// tests: the bound of the batch launches' grid (jxl_debug_tensor_batch_grid), 0: the host's own
int g_batch_grid = 0;
constexpr int64_t kBatchGrid = 65536;  // the host's own bound, k_tensor_resize's
int64_t g_stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // jxl_debug_tensor_batch_stats

// the refusal of item i: its index in front of the reason the single-image entry recorded
jxl_status item_fail(jxl_ctx* c, int i, jxl_status st) {
    const std::string why = jxl_last_error(c);
    char head[48];
    std::snprintf(head, sizeof head, "tensor batch: item %d: ", i);
    return ctx_fail(c, st, (head + why).c_str());
}
jxl_status item_fail(jxl_ctx* c, int i, jxl_status st, const char* why) {
    (void)ctx_fail(c, st, why);
    return item_fail(c, i, st);
}

struct Item {
    ResizeArgs r;
    int tx, ty;  // its tables in the call's set
};

size_t align8(size_t n) { return (n + 7) & ~(size_t)7; }

}  // namespace
}  // namespace jxl

using namespace jxl;

extern "C" {

jxl_status jxl_tensor_resized_batch(jxl_ctx* c, int32_t n, const jxl_tensor_batch_item* items, void* out_device) {
    CtxLink l;
    jxl_status st = ctx_link(c, &l);
    if (st) return st;
    int bad = -1;
    const char* why = batch_check_items(n, items, out_device, &bad);
    if (why) return bad >= 0 ? item_fail(c, bad, JXL_ERR_INVALID_ARGUMENT, why) : ctx_fail(c, JXL_ERR_INVALID_ARGUMENT, why);

    // what the items must agree on, from the pure checks of each (the first refusals of the single-image entries); then the
    // tensors' places and ONE question to the runtime about the whole extent
    BatchShape first{};
    const bool tone = ctx_tone_map_armed(c);  // (all items share the armed block)
    uint64_t bytes_each = 0;
    for (int i = 0; i < n; i++) {
        const jxl_tensor_batch_item& it = items[i];
        TensorLayout lay;
        if ((why = resize_check_params(&it.p, &it.r))) return item_fail(c, i, JXL_ERR_INVALID_ARGUMENT, why);
        jxl_tensor_params q = it.p;  // (the tensor is out_height x out_width: tensor_args' second question)
        q.height = it.r.out_height, q.width = it.r.out_width;
        if ((why = tensor_check_params(&it.p, &lay, tone)) || (why = tensor_check_params(&q, &lay, tone))) return item_fail(c, i, JXL_ERR_INVALID_ARGUMENT, why);
        const BatchShape sh = batch_shape(it.p, it.r, lay);
        if (i == 0) first = sh, bytes_each = lay.bytes;
        else if ((why = batch_check_agree(first, sh))) return item_fail(c, i, JXL_ERR_INVALID_ARGUMENT, why);
    }
    std::vector<uint64_t> off;
    uint64_t total_bytes = 0;
    if ((why = batch_offsets(n, bytes_each, &off, &total_bytes))) return ctx_fail(c, JXL_ERR_INVALID_ARGUMENT, why);
    if ((st = tensor_out_check(c, l, out_device, total_bytes))) return st;

    // per item: the single-image entry's checks, its tables from the call's set, its tile
    const int64_t slots_all = resize_slots(l);
    const int64_t slots = slots_all / n > 1 ? slots_all / n : 1;  // an item's share of the workgroups in flight
    BatchTableSet set;
    std::vector<Item> plan((size_t)n);
    std::vector<ImageHome> homes((size_t)n);
    std::vector<int64_t> tiles((size_t)n);
    std::vector<int> lds((size_t)n);
    int n_color = 0;
    for (int i = 0; i < n; i++) {
        const jxl_tensor_batch_item& it = items[i];
        Item& m = plan[(size_t)i];
        ImageHome& home = homes[(size_t)i];
        switch (it.source) {
            case JXL_BATCH_HOST: home = home_host(it.in, it.alpha), st = JXL_OK; break;
            case JXL_BATCH_RESIDENT: st = ctx_home_resident(c, it.alpha, &home); break;
            default: st = tensor_home_set(c, it.set_id, it.alpha_plane, &it.p, &home);
        }
        if (st) return item_fail(c, i, st);
        TensorLayout lay;
        void* out = (char*)out_device + off[(size_t)i];
        if ((st = resize_args(c, l, &it.p, &it.r, home.in(), home.alpha, out, &m.r, &lay, false))) return item_fail(c, i, st);
        if ((st = tensor_home_fits(c, home, &it.p))) return item_fail(c, i, st);
        if ((m.ty = set.find(0, it.r.box_height, it.r.out_height, it.r.filter, &why)) < 0 ||
            (m.tx = set.find(1, it.r.box_width, it.r.out_width, it.r.filter, &why)) < 0)
            return item_fail(c, i, JXL_ERR_INVALID_ARGUMENT, why);
        if ((st = resize_plan(c, &it.p, &it.r, lay, set.tables[(size_t)m.tx], set.tables[(size_t)m.ty], slots, &m.r))) return item_fail(c, i, st);
        tiles[(size_t)i] = batch_item_tiles(m.r.oh, m.r.ow, m.r.tw, m.r.th);
        lds[(size_t)i] = m.r.lds_bytes;
        n_color = lay.n_color;  // (one value: the items agree on n_out, which is n_color, + 1 with alpha written)
    }
    std::vector<int64_t> base;
    if ((why = batch_tile_base(tiles, &base))) return ctx_fail(c, JXL_ERR_INVALID_ARGUMENT, why);
    const int lds_bytes = batch_lds_bytes(lds);
    const unsigned grid = batch_grid(base[(size_t)n], g_batch_grid > 0 ? g_batch_grid : kBatchGrid);

    // every check has passed: each item's planes to their places, host planes up once per item
    Staged s;
    for (int i = 0; i < n; i++) {
        ResizeArgs& r = plan[(size_t)i].r;
        if ((st = tensor_place(c, homes[(size_t)i], &items[i].p, &r.t.g, &s))) return st;
        resize_set_wide_in(&r);
    }

    // one block: descriptors | tile_base | counts | per table first, off, w
    const size_t at_items = 0, at_base = align8(sizeof(ResizeArgs) * (size_t)n), at_counts = at_base + 8 * ((size_t)n + 1);
    size_t at = at_counts + 8;
    std::vector<size_t> at_table(set.tables.size());
    for (size_t k = 0; k < set.tables.size(); k++) {
        const ResizeTaps& t = set.tables[k];
        at_table[k] = at;
        at += 4 * (t.first.size() + t.off.size() + t.w.size());
    }
    const size_t block = at;
    char* dev = (char*)s.alloc(block);
    if (!dev) return ctx_fail(c, JXL_ERR_OOM, "device allocation failed");
    std::vector<char> pack(block, 0);
    for (size_t k = 0; k < set.tables.size(); k++) {
        const ResizeTaps& t = set.tables[k];
        char* to = pack.data() + at_table[k];
        std::memcpy(to, t.first.data(), 4 * t.first.size());
        std::memcpy(to + 4 * t.first.size(), t.off.data(), 4 * t.off.size());
        std::memcpy(to + 4 * (t.first.size() + t.off.size()), t.w.data(), 4 * t.w.size());
    }
    for (int i = 0; i < n; i++) {
        Item& m = plan[(size_t)i];
        const ResizeTaps &ty = set.tables[(size_t)m.ty], &tx = set.tables[(size_t)m.tx];
        const char *dy = dev + at_table[(size_t)m.ty], *dx = dev + at_table[(size_t)m.tx];
        m.r.yfirst = (const int32_t*)dy, m.r.yoff = (const int32_t*)(dy + 4 * ty.first.size());
        m.r.wy = (const float*)(dy + 4 * (ty.first.size() + ty.off.size()));
        m.r.xfirst = (const int32_t*)dx, m.r.xoff = (const int32_t*)(dx + 4 * tx.first.size());
        m.r.wx = (const float*)(dx + 4 * (tx.first.size() + tx.off.size()));
        std::memcpy(pack.data() + at_items + sizeof(ResizeArgs) * (size_t)i, &m.r, sizeof(ResizeArgs));
    }
    std::memcpy(pack.data() + at_base, base.data(), 8 * ((size_t)n + 1));
    const int32_t counts[2] = {n, (int32_t)set.tables.size()};
    std::memcpy(pack.data() + at_counts, counts, 8);
    TENSOR_HIP(c, hipMemcpy(dev, pack.data(), block, hipMemcpyHostToDevice));
    const int64_t stats[8] = {set.asked, (int64_t)set.tables.size(), (int64_t)block, base[(size_t)n], grid, lds_bytes, plan[0].r.tw, plan[0].r.th};
    std::memcpy(g_stats, stats, sizeof stats);
    launch_tensor_resize_batch((const ResizeArgs*)(dev + at_items), (const int64_t*)(dev + at_base), (const int32_t*)(dev + at_counts),
                               first.dtype, n_color, grid, lds_bytes, l.stream);
    TENSOR_HIP(c, hipStreamSynchronize(l.stream));
    TENSOR_HIP(c, hipGetLastError());
    return JXL_OK;
}

// tests: the bound of the grid of the batch launches that follow, 0 for the host's own again (one workgroup then walks tiles of
// several items)
jxl_status jxl_debug_tensor_batch_grid(int32_t n) {
    if (n < 0) return JXL_ERR_INVALID_ARGUMENT;
    g_batch_grid = n;
    return JXL_OK;
}

// measurements: what the last batch call that launched planned -- table lookups, tables built (the difference was shared), bytes
// of the one transfer, tiles, grid, LDS bytes, and the first item's tile
jxl_status jxl_debug_tensor_batch_stats(int64_t out[8]) {
    if (!out) return JXL_ERR_INVALID_ARGUMENT;
    for (int i = 0; i < 8; i++) out[i] = g_stats[i];
    return JXL_OK;
}

}  // extern "C"
