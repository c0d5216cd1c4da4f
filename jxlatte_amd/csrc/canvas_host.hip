// Device plane sets: the canvas and the reference frames of JXLCodestreamDecoder.decode (JXLCodestreamDecoder.java:640-657) kept
// on the device, and blendFrame (:515-537) on them as one launch (k_canvas.hip). A set is ONE allocation, its planes a multiple
// of 256 bytes apart, so every plane starts 16-byte aligned; a cast rewrites a plane in place (both kinds of sample are 4
// bytes wide). The context (host.hip) lends its stream and its resident planes through jxl_internal.h's ctx_* functions.
// Ordering: everything here is queued on the context's stream except the transfers to and from the host, which wait for the
// stream first and are complete on return (the stream does not synchronise with the null stream).
#include "jxl_internal.h"
#include "canvas_check.h"
#include "canvas_patch_check.h"
#include "modplanes_check.h"
#include "pfm_check.h"

#include <cstring>
#include <new>

namespace jxl {

struct CanvasSet {
    int32_t n = 0, h = 0, w = 0;
    int32_t type[JXL_CANVAS_MAX_PLANES] = {};
    size_t stride = 0;  // bytes between planes
    char* base = nullptr;
    uint32_t* plane(int i) const { return reinterpret_cast<uint32_t*>(base + stride * (size_t)i); }
    size_t plane_bytes() const { return 4 * (size_t)h * (size_t)w; }
};
struct CanvasStore {
    std::vector<CanvasSet*> sets;  // index = id; a destroyed set leaves a null its id is handed out again from
};

void canvas_store_free(CanvasStore* s) {
    if (!s) return;
    for (CanvasSet* k : s->sets)
        if (k) {
            (void)hipFree(k->base);
            delete k;
        }
    delete s;
}

bool canvas_view(const CanvasStore* s, int32_t id, CanvasView* out) {
    const CanvasSet* k = (s && id >= 0 && (size_t)id < s->sets.size()) ? s->sets[(size_t)id] : nullptr;
    if (!k) return false;
    out->n = k->n, out->h = k->h, out->w = k->w;
    for (int i = 0; i < JXL_CANVAS_MAX_PLANES; i++) {
        out->type[i] = i < k->n ? k->type[i] : 0;
        out->plane[i] = i < k->n ? k->plane(i) : nullptr;
    }
    return true;
}

namespace {

#define CV_HIP(c, expr)                                                                                                       \
    do {                                                                                                                      \
        hipError_t e_ = (expr);                                                                                               \
        if (e_ != hipSuccess) return ctx_fail(c, e_ == hipErrorOutOfMemory ? JXL_ERR_OOM : JXL_ERR_DEVICE, hipGetErrorString(e_)); \
    } while (0)

CanvasSet* find(const CtxLink& l, int32_t id) {
    CanvasStore* s = *l.canvas;
    return (s && id >= 0 && (size_t)id < s->sets.size()) ? s->sets[(size_t)id] : nullptr;
}

// a new set of n planes (contents undefined), registered under *id
jxl_status new_set(jxl_ctx* c, const CtxLink& l, int32_t n, int32_t h, int32_t w, const int32_t* types, CanvasSet** out, int32_t* id) {
    if (n > JXL_CANVAS_MAX_PLANES) return ctx_fail(c, JXL_ERR_UNSUPPORTED, "canvas: more than 16 planes");
    if (n < 1 || h < 1 || w < 1 || !types || !id) return ctx_fail(c, JXL_ERR_INVALID_ARGUMENT, "canvas: bad arguments");
    for (int i = 0; i < n; i++)
        if (types[i] != JXL_PLANE_FLOAT && types[i] != JXL_PLANE_INT32) return ctx_fail(c, JXL_ERR_INVALID_ARGUMENT, "canvas: plane type");
    CanvasSet* k = nullptr;
    try {
        if (!*l.canvas) *l.canvas = new CanvasStore();
        k = new CanvasSet();
        std::vector<CanvasSet*>& v = (*l.canvas)->sets;
        size_t slot = 0;
        while (slot < v.size() && v[slot]) slot++;
        if (slot == v.size()) v.push_back(nullptr);
        k->n = n, k->h = h, k->w = w;
        for (int i = 0; i < n; i++) k->type[i] = types[i];
        k->stride = (k->plane_bytes() + 255) & ~(size_t)255;
        if (hipMalloc(reinterpret_cast<void**>(&k->base), k->stride * (size_t)n) != hipSuccess) {
            (void)hipGetLastError();
            delete k;
            return ctx_fail(c, JXL_ERR_OOM, "device allocation failed (plane set)");
        }
        v[slot] = k;
        *id = (int32_t)slot;
    } catch (const std::bad_alloc&) {
        delete k;
        return ctx_fail(c, JXL_ERR_OOM, "canvas: host allocation failed");
    }
    *out = k;
    return JXL_OK;
}

// The settled result list of the Modular context, checked against `d` (modplanes_check.h); upsampled: for
// jxl_canvas_from_modular_up, with its factor and weights. Nothing has been queued when this refuses.
jxl_status modular_results(jxl_ctx* c, const jxl_modular_planes_desc* d, bool upsampled, int32_t up, const float* weights,
                           std::vector<ModResult>* res) {
    bool ran = false;
    jxl_status st = ctx_modular_out(c, res, &ran);  // (settled: a speculative plan has been verified or redone)
    if (st) return st;
    ModPlaneShape shapes[64];
    std::vector<ModPlaneShape> more;
    ModPlaneShape* sh = shapes;
    try {
        if (res->size() > 64) more.resize(res->size()), sh = more.data();
    } catch (const std::bad_alloc&) {
        return ctx_fail(c, JXL_ERR_OOM, "canvas: host allocation failed");
    }
    for (size_t i = 0; i < res->size(); i++) sh[i] = ModPlaneShape{(*res)[i].h, (*res)[i].w};
    const char* why = "";
    st = !upsampled ? modplanes_check(d, sh, (int32_t)res->size(), ran, &why)
                    : modplanes_up_check(d, sh, (int32_t)res->size(), ran, up, weights != nullptr, &why);
    return st ? ctx_fail(c, st, why) : JXL_OK;
}

void shape_of(const CanvasSet* k, jxl_canvas_shape* s) {
    s->n = k->n, s->h = k->h, s->w = k->w;
    for (int i = 0; i < JXL_CANVAS_MAX_PLANES; i++) s->types[i] = i < k->n ? k->type[i] : 0;
}

}  // namespace
}  // namespace jxl

using namespace jxl;

extern "C" {

jxl_status jxl_canvas_create(jxl_ctx* c, int32_t n, int32_t h, int32_t w, const int32_t* types, int32_t* id) {
    CtxLink l;
    jxl_status st = ctx_link(c, &l);
    if (st) return st;
    CanvasSet* k;
    if ((st = new_set(c, l, n, h, w, types, &k, id))) return st;
    CV_HIP(c, hipMemsetAsync(k->base, 0, k->stride * (size_t)k->n, l.stream));
    return JXL_OK;
}

jxl_status jxl_canvas_destroy(jxl_ctx* c, int32_t id) {
    CtxLink l;
    jxl_status st = ctx_link(c, &l);
    if (st) return st;
    CanvasSet* k = find(l, id);
    if (!k) return ctx_fail(c, JXL_ERR_INVALID_ARGUMENT, "canvas: unknown set");
    CV_HIP(c, hipStreamSynchronize(l.stream));  // a queued launch may still use the planes
    (void)hipFree(k->base);
    delete k;
    (*l.canvas)->sets[(size_t)id] = nullptr;
    return JXL_OK;
}

jxl_status jxl_canvas_describe(jxl_ctx* c, int32_t id, jxl_canvas_shape* out) {
    CtxLink l;
    jxl_status st = ctx_link(c, &l);
    if (st) return st;
    const CanvasSet* k = find(l, id);
    if (!k || !out) return ctx_fail(c, JXL_ERR_INVALID_ARGUMENT, "canvas: unknown set");
    shape_of(k, out);
    return JXL_OK;
}

jxl_status jxl_canvas_clone(jxl_ctx* c, int32_t id, int32_t* new_id) {
    CtxLink l;
    jxl_status st = ctx_link(c, &l);
    if (st) return st;
    const CanvasSet* k = find(l, id);
    if (!k || !new_id) return ctx_fail(c, JXL_ERR_INVALID_ARGUMENT, "canvas: unknown set");
    CanvasSet* q;
    if ((st = new_set(c, l, k->n, k->h, k->w, k->type, &q, new_id))) return st;
    CV_HIP(c, hipMemcpyAsync(q->base, k->base, k->stride * (size_t)k->n, hipMemcpyDeviceToDevice, l.stream));
    return JXL_OK;
}

jxl_status jxl_canvas_upload(jxl_ctx* c, int32_t id, int32_t plane, const void* src, int32_t type) {
    CtxLink l;
    jxl_status st = ctx_link(c, &l);
    if (st) return st;
    CanvasSet* k = find(l, id);
    if (!k) return ctx_fail(c, JXL_ERR_INVALID_ARGUMENT, "canvas: unknown set");
    if (plane < 0 || plane >= k->n || !src || (type != JXL_PLANE_FLOAT && type != JXL_PLANE_INT32))
        return ctx_fail(c, JXL_ERR_INVALID_ARGUMENT, "canvas upload: bad arguments");
    CV_HIP(c, hipStreamSynchronize(l.stream));
    CV_HIP(c, hipMemcpy(k->plane(plane), src, k->plane_bytes(), hipMemcpyHostToDevice));
    k->type[plane] = type;
    return JXL_OK;
}

jxl_status jxl_canvas_download(jxl_ctx* c, int32_t id, int32_t plane, void* dst, int32_t* type) {
    CtxLink l;
    jxl_status st = ctx_link(c, &l);
    if (st) return st;
    const CanvasSet* k = find(l, id);
    if (!k) return ctx_fail(c, JXL_ERR_INVALID_ARGUMENT, "canvas: unknown set");
    if (plane < 0 || plane >= k->n || !dst) return ctx_fail(c, JXL_ERR_INVALID_ARGUMENT, "canvas download: bad arguments");
    CV_HIP(c, hipStreamSynchronize(l.stream));
    CV_HIP(c, hipGetLastError());
    CV_HIP(c, hipMemcpy(dst, k->plane(plane), k->plane_bytes(), hipMemcpyDeviceToHost));
    if (type) *type = k->type[plane];
    return JXL_OK;
}

jxl_status jxl_canvas_from_planes(jxl_ctx* c, int32_t n_extra, const int32_t* extra_types, int32_t* id) {
    CtxLink l;
    jxl_status st = ctx_link(c, &l);
    if (st) return st;
    int h, w;
    float* p[3];
    if ((st = ctx_planes_get(c, &h, &w, p))) return st;
    if (n_extra > JXL_CANVAS_MAX_PLANES - 3) return ctx_fail(c, JXL_ERR_UNSUPPORTED, "canvas: more than 16 planes");
    if (n_extra < 0 || (n_extra > 0 && !extra_types)) return ctx_fail(c, JXL_ERR_INVALID_ARGUMENT, "canvas: bad arguments");
    int32_t types[JXL_CANVAS_MAX_PLANES] = {JXL_PLANE_FLOAT, JXL_PLANE_FLOAT, JXL_PLANE_FLOAT};
    for (int i = 0; i < n_extra; i++) types[3 + i] = extra_types[i];
    CanvasSet* k;
    if ((st = new_set(c, l, 3 + n_extra, h, w, types, &k, id))) return st;
    for (int i = 0; i < 3; i++) CV_HIP(c, hipMemcpyAsync(k->plane(i), p[i], k->plane_bytes(), hipMemcpyDeviceToDevice, l.stream));
    if (n_extra > 0) CV_HIP(c, hipMemsetAsync(k->plane(3), 0, k->stride * (size_t)n_extra, l.stream));
    return JXL_OK;
}

jxl_status jxl_canvas_cast(jxl_ctx* c, int32_t id, int32_t plane, int32_t depth) {
    CtxLink l;
    jxl_status st = ctx_link(c, &l);
    if (st) return st;
    CanvasSet* k = find(l, id);
    if (!k) return ctx_fail(c, JXL_ERR_INVALID_ARGUMENT, "canvas: unknown set");
    if (plane < 0 || plane >= k->n) return ctx_fail(c, JXL_ERR_INVALID_ARGUMENT, "canvas cast: bad plane");
    if (k->type[plane] == JXL_PLANE_FLOAT) return JXL_OK;  // ImageBuffer.java:100-101
    const int32_t max = pfm_depth_max(depth);
    if (max < 1) return ctx_fail(c, JXL_ERR_INVALID_ARGUMENT, "invalid Max Value");  // ImageBuffer.java:115-116
    // castToFloat0 (ImageBuffer.java:112-127) element by element, in place: the kernel of jxl_stage_modular_to_float
    launch_modular_to_float(reinterpret_cast<const int32_t*>(k->plane(plane)), nullptr, (int64_t)k->h * k->w, 1.0f / (float)max,
                            reinterpret_cast<float*>(k->plane(plane)), l.stream);
    CV_HIP(c, hipGetLastError());
    k->type[plane] = JXL_PLANE_FLOAT;
    return JXL_OK;
}

jxl_status jxl_canvas_cast_planes(jxl_ctx* c, int32_t n, const jxl_canvas_cast_item* items) {
    CtxLink l;
    jxl_status st = ctx_link(c, &l);
    if (st) return st;
    jxl_canvas_shape sh;  // (the check looks at one item's set at a time)
    float scale[kCanvasMaxCasts];
    const char* why = "";
    auto lookup = [&](int32_t id) -> const jxl_canvas_shape* {
        const CanvasSet* k = find(l, id);
        if (!k) return nullptr;
        shape_of(k, &sh);
        return &sh;
    };
    if ((st = canvas_cast_list_check(n, items, lookup, scale, &why))) return ctx_fail(c, st, why);
    CastArgs a{};
    int64_t blocks = 0;
    for (int32_t i = 0; i < n; i++) {
        if (scale[i] == 0.0f) continue;
        const CanvasSet* k = find(l, items[i].set);
        CastItem& q = a.it[a.n];
        q.base = k->plane(items[i].plane);
        q.n = (int64_t)k->h * k->w;
        q.scale = scale[i];
        a.first_block[a.n++] = (int32_t)blocks;
        blocks += (q.n + kCastRun - 1) / kCastRun;
        if (blocks > INT32_MAX) return ctx_fail(c, JXL_ERR_UNSUPPORTED, "canvas cast: the planes do not fit one launch");
    }
    a.first_block[a.n] = (int32_t)blocks;
    launch_canvas_cast(a, l.stream);
    CV_HIP(c, hipGetLastError());
    for (int32_t i = 0; i < n; i++) find(l, items[i].set)->type[items[i].plane] = JXL_PLANE_FLOAT;
    return JXL_OK;
}

jxl_status jxl_canvas_patches_check(const jxl_patch_desc* d, const jxl_canvas_shape* frame, int32_t colors_resident,
                                    const jxl_canvas_shape* const ref[4], int32_t* first_bad) {
    const char* why = "";
    bool aliased = false;
    for (int k = 0; ref && k < 4; k++) aliased = aliased || (ref[k] && ref[k] == frame);
    try {
        PatchStage ps;
        const jxl_status st = canvas_patches_check(d, frame, colors_resident, ref, aliased, &ps, &why, first_bad);
        return st ? ctx_fail(nullptr, st, why) : JXL_OK;
    } catch (const std::bad_alloc&) {
        return ctx_fail(nullptr, JXL_ERR_OOM, "patches: host allocation failed");
    }
}

jxl_status jxl_canvas_patches(jxl_ctx* c, const jxl_patch_desc* d, int32_t frame_set, int32_t colors_resident, const int32_t ref_set[4]) {
    CtxLink l;
    jxl_status st = ctx_link(c, &l);
    if (st) return st;
    if (!d || !ref_set) return ctx_fail(c, JXL_ERR_INVALID_ARGUMENT, "canvas patches: null argument");
    const CanvasSet* fr = find(l, frame_set);
    const CanvasSet* rf[4];
    jxl_canvas_shape sf, sr[4];
    const jxl_canvas_shape* srp[4];
    bool aliased = false;
    if (!fr) return ctx_fail(c, JXL_ERR_INVALID_ARGUMENT, "canvas: unknown set");
    shape_of(fr, &sf);
    for (int k = 0; k < 4; k++) {
        rf[k] = ref_set[k] == -1 ? nullptr : find(l, ref_set[k]);
        if (ref_set[k] != -1 && !rf[k]) return ctx_fail(c, JXL_ERR_INVALID_ARGUMENT, "canvas: unknown set");
        if (rf[k]) shape_of(rf[k], &sr[k]);
        srp[k] = rf[k] ? &sr[k] : nullptr;
        aliased = aliased || rf[k] == fr;
    }
    const char* why = "";
    const char* dev = nullptr;
    PatchStage ps;
    size_t off_ops, off_tile, off_start, off_list, off_planes;
    try {
        if ((st = canvas_patches_check(d, &sf, colors_resident, srp, aliased, &ps, &why, nullptr))) return ctx_fail(c, st, why);
        float* rp[3] = {nullptr, nullptr, nullptr};
        if (colors_resident) {
            int h = 0, w = 0;
            if ((st = ctx_planes_get(c, &h, &w, rp))) return st;
            if (h != fr->h || w != fr->w) return ctx_fail(c, JXL_ERR_INVALID_ARGUMENT, "canvas: the resident planes have another size than the set");
        }
        if (ps.bins.tile.empty()) return JXL_OK;
        // the tables, back to back in the page-locked staging buffer: one transfer (the layout of jxl_stage_patches)
        const int n_chan = ps.n_chan;
        auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
        off_ops = up(ps.rec.size() * sizeof(PatchRec));
        off_tile = off_ops + up(ps.ops.size() * sizeof(PatchOp));
        off_start = off_tile + up(ps.bins.tile.size() * 4);
        off_list = off_start + up(ps.bins.start.size() * 4);
        off_planes = off_list + up(ps.bins.list.size() * 4);
        const size_t total = off_planes + up(((size_t)n_chan * 5 + 4) * 8);
        char* h_tab = nullptr;
        if ((st = ctx_tables_reserve(c, total, &h_tab))) return st;
        memcpy(h_tab, ps.rec.data(), ps.rec.size() * sizeof(PatchRec));
        memcpy(h_tab + off_ops, ps.ops.data(), ps.ops.size() * sizeof(PatchOp));
        memcpy(h_tab + off_tile, ps.bins.tile.data(), ps.bins.tile.size() * 4);
        memcpy(h_tab + off_start, ps.bins.start.data(), ps.bins.start.size() * 4);
        memcpy(h_tab + off_list, ps.bins.list.data(), ps.bins.list.size() * 4);
        int64_t* tab = reinterpret_cast<int64_t*>(h_tab + off_planes);
        for (int ch = 0; ch < n_chan; ch++)
            tab[ch] = (int64_t)reinterpret_cast<intptr_t>(colors_resident && ch < 3 ? reinterpret_cast<uint32_t*>(rp[ch]) : fr->plane(ch));
        for (int k = 0; k < 4; k++) {
            for (int ch = 0; ch < n_chan; ch++) tab[n_chan * (1 + k) + ch] = rf[k] ? (int64_t)reinterpret_cast<intptr_t>(rf[k]->plane(ch)) : 0;
            tab[n_chan * 5 + k] = rf[k] ? rf[k]->w : 0;
        }
        if ((st = ctx_tables_send(c, total, &dev))) return st;
    } catch (const std::bad_alloc&) {
        return ctx_fail(c, JXL_ERR_OOM, "patches: host allocation failed");
    }
    launch_patches(reinterpret_cast<const int64_t*>(dev + off_planes), ps.n_chan, fr->w, reinterpret_cast<const PatchRec*>(dev),
                   reinterpret_cast<const PatchOp*>(dev + off_ops), reinterpret_cast<const int32_t*>(dev + off_tile),
                   reinterpret_cast<const int32_t*>(dev + off_start), reinterpret_cast<const int32_t*>(dev + off_list),
                   (int)ps.bins.tile.size(), ps.bins.tiles_x, l.stream);
    CV_HIP(c, hipGetLastError());
    return JXL_OK;
}

jxl_status jxl_canvas_blend_check(const jxl_canvas_blend_desc* d, const jxl_canvas_shape* canvas, const jxl_canvas_shape* frame,
                                  const jxl_canvas_shape* ref) {
    const char* why = "";
    const jxl_status st = canvas_blend_check(d, canvas, frame, ref, nullptr, &why);
    return st ? ctx_fail(nullptr, st, why) : JXL_OK;
}

jxl_status jxl_canvas_blend(jxl_ctx* c, const jxl_canvas_blend_desc* d) {
    CtxLink l;
    jxl_status st = ctx_link(c, &l);
    if (st) return st;
    if (!d) return ctx_fail(c, JXL_ERR_INVALID_ARGUMENT, "canvas blend: null argument");
    const CanvasSet *cv = find(l, d->canvas), *fr = find(l, d->frame), *rf = d->ref >= 0 ? find(l, d->ref) : nullptr;
    if (!cv || !fr || (d->ref >= 0 && !rf)) return ctx_fail(c, JXL_ERR_INVALID_ARGUMENT, "canvas: unknown set");
    jxl_canvas_shape sc, sf, sr;
    shape_of(cv, &sc);
    shape_of(fr, &sf);
    if (rf) shape_of(rf, &sr);
    CanvasChanOp ops[JXL_CANVAS_MAX_PLANES];
    const char* why = "";
    if ((st = canvas_blend_check(d, &sc, &sf, rf ? &sr : nullptr, ops, &why))) return ctx_fail(c, st, why);
    const jxl_blend_rect& r = d->rect;
    if (r.h == 0 || r.w == 0) return JXL_OK;
    CanvasArgs a{};
    a.n = cv->n, a.h = r.h, a.w = r.w;
    a.cw = cv->w, a.fw = fr->w, a.rw = rf ? rf->w : 0;
    const int64_t c_off = (int64_t)r.canvas_y * cv->w + r.canvas_x, f_off = (int64_t)r.frame_y * fr->w + r.frame_x;
    const int64_t r_off = rf ? (int64_t)r.ref_y * rf->w + r.ref_x : 0, rf_off = rf ? (int64_t)r.frame_y * rf->w + r.frame_x : 0;
    a.c_align = (int32_t)(c_off & 3);
    for (int ch = 0; ch < cv->n; ch++) {
        const jxl_canvas_blend_chan& k = d->chan[ch];
        const CanvasChanOp& o = ops[ch];
        CanvasChan& q = a.ch[ch];
        q.canvas = cv->plane(ch) + c_off;
        q.frame = o.frame ? fr->plane(k.frame_plane) + f_off : nullptr;
        q.ref = o.ref ? rf->plane(ch) + (o.frame ? r_off : rf_off) : nullptr;  // (blendMulAdd's alpha copy reads at frameOffset, :390)
        q.frame_alpha = o.frame_alpha ? fr->plane(k.frame_alpha) + f_off : nullptr;
        q.ref_alpha = o.ref_alpha ? rf->plane(k.ref_alpha) + r_off : nullptr;
        q.op = o.op;
        q.flags = (int32_t)k.flags;
    }
    launch_canvas_blend(a, l.stream);
    CV_HIP(c, hipGetLastError());
    return JXL_OK;
}

jxl_status jxl_canvas_from_modular(jxl_ctx* c, const jxl_modular_planes_desc* d, int32_t* id) {
    CtxLink l;
    jxl_status st = ctx_link(c, &l);
    if (st) return st;
    std::vector<ModResult> res;
    if ((st = modular_results(c, d, false, 0, nullptr, &res))) return st;
    if (!id) return ctx_fail(c, JXL_ERR_INVALID_ARGUMENT, "canvas: bad arguments");
    int32_t types[JXL_CANVAS_MAX_PLANES];
    for (int i = 0; i < d->n_planes; i++) types[i] = d->plane[i].type;
    CanvasSet* k;
    int32_t new_id = -1;
    if ((st = new_set(c, l, d->n_planes, d->height, d->width, types, &k, &new_id))) return st;
    ModPlanesArgs a{};
    a.h = d->height, a.w = d->width, a.n = d->n_planes;
    for (int i = 0; i < d->n_planes; i++) {
        const jxl_modular_plane& p = d->plane[i];
        ModPlane& q = a.p[i];
        q.a = res[(size_t)p.channel].d;
        q.b = p.add_channel >= 0 ? res[(size_t)p.add_channel].d : nullptr;
        q.out = k->plane(i);
        q.pitch = res[(size_t)p.channel].w;
        q.is_float = p.type == JXL_PLANE_FLOAT ? 1 : 0;
        q.scale = p.scale;
    }
    launch_modplanes(a, l.stream);
    CV_HIP(c, hipGetLastError());
    *id = new_id;
    return JXL_OK;
}

jxl_status jxl_canvas_from_modular_up(jxl_ctx* c, const jxl_modular_planes_desc* d, int32_t up, const float* weights, int32_t* id) {
    CtxLink l;
    jxl_status st = ctx_link(c, &l);
    if (st) return st;
    std::vector<ModResult> res;
    if ((st = modular_results(c, d, true, up, weights, &res))) return st;
    if (!id) return ctx_fail(c, JXL_ERR_INVALID_ARGUMENT, "canvas: bad arguments");
    // the weights go up first: nothing is left behind when their allocation fails
    const size_t wbytes = sizeof(float) * 25 * (size_t)up * (size_t)up;
    float* dw = nullptr;
    if (hipMalloc(reinterpret_cast<void**>(&dw), wbytes) != hipSuccess) {
        (void)hipGetLastError();
        return ctx_fail(c, JXL_ERR_OOM, "device allocation failed (upsampling weights)");
    }
    if (hipMemcpy(dw, weights, wbytes, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipGetLastError();
        (void)hipFree(dw);
        return ctx_fail(c, JXL_ERR_DEVICE, "upload of the upsampling weights failed");
    }
    int32_t types[JXL_CANVAS_MAX_PLANES];
    for (int i = 0; i < d->n_planes; i++) types[i] = JXL_PLANE_FLOAT;
    CanvasSet* k;
    int32_t new_id = -1;
    if ((st = new_set(c, l, d->n_planes, d->height * up, d->width * up, types, &k, &new_id))) {
        (void)hipFree(dw);
        return st;
    }
    ModUpArgs a{};
    a.h = d->height, a.w = d->width, a.n = d->n_planes;
    a.weights = dw;
    for (int i = 0; i < d->n_planes; i++) {
        const jxl_modular_plane& p = d->plane[i];
        ModUpPlane& q = a.p[i];
        q.a = res[(size_t)p.channel].d;
        q.b = p.add_channel >= 0 ? res[(size_t)p.add_channel].d : nullptr;
        q.out = reinterpret_cast<float*>(k->plane(i));
        q.pitch = res[(size_t)p.channel].w;
        q.scale = p.scale;
    }
    launch_modplanes_up(a, up, l.stream);
    const hipError_t e = hipGetLastError();
    const hipError_t e2 = hipStreamSynchronize(l.stream);  // the weights are freed on return, as jxl_planes_upsample frees its own
    (void)hipFree(dw);
    if (e != hipSuccess || e2 != hipSuccess) return ctx_fail(c, JXL_ERR_DEVICE, hipGetErrorString(e != hipSuccess ? e : e2));
    *id = new_id;
    return JXL_OK;
}

jxl_status jxl_canvas_orient(jxl_ctx* c, int32_t id, int32_t orientation) {
    CtxLink l;
    jxl_status st = ctx_link(c, &l);
    if (st) return st;
    CanvasSet* k = find(l, id);
    if (!k) return ctx_fail(c, JXL_ERR_INVALID_ARGUMENT, "canvas: unknown set");
    if (orientation < 1 || orientation > 8) return ctx_fail(c, JXL_ERR_STATE, "orientation outside 1..8");  // as jxl_planes_orient
    if (orientation == 1) return JXL_OK;
    // out of place, into a new allocation of the same layout (h * w is the same either way round); the old one is freed once
    // the stream has passed the launches that read it
    char* base = nullptr;
    if (hipMalloc(reinterpret_cast<void**>(&base), k->stride * (size_t)k->n) != hipSuccess) {
        (void)hipGetLastError();
        return ctx_fail(c, JXL_ERR_OOM, "device allocation failed (plane set)");
    }
    for (int i = 0; i < k->n; i++) launch_orient(k->plane(i), k->h, k->w, orientation, base + k->stride * (size_t)i, l.stream);
    const hipError_t e = hipGetLastError();
    const hipError_t e2 = hipStreamSynchronize(l.stream);
    if (e != hipSuccess || e2 != hipSuccess) {
        (void)hipFree(base);
        return ctx_fail(c, JXL_ERR_DEVICE, hipGetErrorString(e != hipSuccess ? e : e2));
    }
    (void)hipFree(k->base);
    k->base = base;
    if (orientation > 4) std::swap(k->h, k->w);
    return JXL_OK;
}

jxl_status jxl_canvas_to_planes(jxl_ctx* c, int32_t id) {
    CtxLink l;
    jxl_status st = ctx_link(c, &l);
    if (st) return st;
    const CanvasSet* k = find(l, id);
    if (!k) return ctx_fail(c, JXL_ERR_INVALID_ARGUMENT, "canvas: unknown set");
    if (k->n < 3 || k->type[0] != JXL_PLANE_FLOAT || k->type[1] != JXL_PLANE_FLOAT || k->type[2] != JXL_PLANE_FLOAT)
        return ctx_fail(c, JXL_ERR_STATE, "canvas: the first three planes are not float planes");
    CV_HIP(c, hipStreamSynchronize(l.stream));  // (the resident planes may be reallocated below)
    float* p[3];
    if ((st = ctx_planes_set(c, k->h, k->w, p))) return st;
    for (int i = 0; i < 3; i++) CV_HIP(c, hipMemcpyAsync(p[i], k->plane(i), k->plane_bytes(), hipMemcpyDeviceToDevice, l.stream));
    return JXL_OK;
}

jxl_status jxl_canvas_take_planes(jxl_ctx* c, int32_t id) {
    CtxLink l;
    jxl_status st = ctx_link(c, &l);
    if (st) return st;
    CanvasSet* k = find(l, id);
    jxl_canvas_shape sk;
    if (k) shape_of(k, &sk);
    int h = 0, w = 0;
    float* p[3];
    if (k && ctx_planes_get(c, &h, &w, p) != JXL_OK) h = w = 0;
    const char* why = "";
    if ((st = canvas_take_check(k ? &sk : nullptr, h, w, &why))) return ctx_fail(c, st, why);
    for (int i = 0; i < 3; i++) {
        CV_HIP(c, hipMemcpyAsync(k->plane(i), p[i], k->plane_bytes(), hipMemcpyDeviceToDevice, l.stream));
        k->type[i] = JXL_PLANE_FLOAT;
    }
    return JXL_OK;
}

}  // extern "C"
