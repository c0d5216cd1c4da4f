// Host side of the resized tensor exit (k_tensor_resize.hip): the three jxl_*_tensor_resized entries beside their unresized
// siblings (tensor_host.hip), whose checks of the parameters, the planes and out_device they share (tensor_args). Their own pure
// part -- box, size, filter, the tap tables, the tile -- is tensor_resize_check.h's. Nothing is queued before every check has
// passed; the tables go up once per call, in one transfer; the stream is synchronised before return.
// Each entry resolves its image's home (image_home.h, in the words of tensor_host.hip) and calls resized_from_home. The plan of a
// launch is a function of tensor_host.h: the batch entry (tensor_batch_host.hip) plans each item with it.
#include "tensor_host.h"
#include "tensor_resize_check.h"

#include <cstring>

namespace jxl {
namespace {

// tests: the tile and the LDS skew of the launches that follow (jxl_debug_tensor_resize_tile, jxl_debug_tensor_resize_skew)
int g_force_tw = 0, g_force_th = 0;
bool g_skew = true;

struct Tables {
    ResizeTaps x, y;
};

// the tables of one image
jxl_status resize_tables(jxl_ctx* c, const jxl_resize_params* rz, Tables* tb) {
    const char* why = resize_build_taps(rz->box_height, rz->out_height, rz->filter, &tb->y);
    if (!why) why = resize_build_taps(rz->box_width, rz->out_width, rz->filter, &tb->x);
    return why ? ctx_fail(c, JXL_ERR_INVALID_ARGUMENT, why) : JXL_OK;
}

// the tables to the device in one transfer, the launch, the synchronisation (the plane pointers of r->t are set)
jxl_status resize_run(jxl_ctx* c, const CtxLink& l, ResizeArgs* r, const Tables& tb, Staged* s) {
    const std::vector<int32_t>* iv[4] = {&tb.y.first, &tb.y.off, &tb.x.first, &tb.x.off};
    size_t words = tb.y.w.size() + tb.x.w.size();
    for (const auto* v : iv) words += v->size();
    std::vector<uint32_t> pack(words);
    size_t at = 0, where[6];
    for (int i = 0; i < 4; i++) {
        where[i] = at;
        std::memcpy(pack.data() + at, iv[i]->data(), iv[i]->size() * 4);
        at += iv[i]->size();
    }
    where[4] = at;
    std::memcpy(pack.data() + at, tb.y.w.data(), tb.y.w.size() * 4);
    at += tb.y.w.size();
    where[5] = at;
    std::memcpy(pack.data() + at, tb.x.w.data(), tb.x.w.size() * 4);
    const uint32_t* d = (const uint32_t*)s->up(pack.data(), words * 4);
    if (!d) return ctx_fail(c, JXL_ERR_OOM, "device allocation failed");
    r->yfirst = (const int32_t*)(d + where[0]), r->yoff = (const int32_t*)(d + where[1]);
    r->xfirst = (const int32_t*)(d + where[2]), r->xoff = (const int32_t*)(d + where[3]);
    r->wy = (const float*)(d + where[4]), r->wx = (const float*)(d + where[5]);
    resize_set_wide_in(r);
    launch_tensor_resize(*r, l.stream);
    TENSOR_HIP(c, hipStreamSynchronize(l.stream));
    TENSOR_HIP(c, hipGetLastError());
    return JXL_OK;
}

// the body of the three entries: resize_args, the tables and the plan of a single image, the home's second half, the planes'
// places, the launch
jxl_status resized_from_home(jxl_ctx* c, const CtxLink& l, const ImageHome& m, const jxl_tensor_params* p, const jxl_resize_params* rz,
                             void* out) {
    ResizeArgs r;
    TensorLayout lay;
    Tables tb;
    jxl_status st = resize_args(c, l, p, rz, m.in(), m.alpha, out, &r, &lay);
    if (st || (st = resize_tables(c, rz, &tb))) return st;
    if ((st = resize_plan(c, p, rz, lay, tb.x, tb.y, resize_slots(l), &r))) return st;
    if ((st = tensor_home_fits(c, m, p))) return st;
    Staged s;
    if ((st = tensor_place(c, m, p, &r.t.g, &s))) return st;
    return resize_run(c, l, &r, tb, &s);
}

}  // namespace

int64_t resize_slots(const CtxLink& l) {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, l.device) != hipSuccess) cus = 0, (void)hipGetLastError();
    return 2 * (int64_t)cus;
}

jxl_status resize_plan(jxl_ctx* c, const jxl_tensor_params* p, const jxl_resize_params* rz, const TensorLayout& lay, const ResizeTaps& x,
                       const ResizeTaps& y, int64_t slots, ResizeArgs* r) {
    r->planes = lay.n_color + (tensor_alpha_read(p) ? 1 : 0);
    ResizeTile tile;
    const char* why = resize_pick_tile(x, rz->box_x0, y, r->planes, g_skew, slots, g_force_tw, g_force_th, &tile);
    if (why) return ctx_fail(c, JXL_ERR_INVALID_ARGUMENT, why);
    r->src_w = p->width;
    r->x0 = rz->box_x0, r->y0 = rz->box_y0;
    r->oh = rz->out_height, r->ow = rz->out_width;
    r->tw = tile.tw, r->th = tile.th;
    r->lds_w = tile.lds_w, r->lds_bytes = tile.lds_bytes;
    r->skew = g_skew ? 1 : 0;
    return JXL_OK;
}

void resize_set_wide_in(ResizeArgs* r) {
    uint64_t bases[4];
    int nb = 0;
    for (int i = 0; i < r->t.g.c.n_planes; i++) bases[nb++] = (uint64_t)(uintptr_t)r->t.g.c.in[i];
    if (r->t.g.alpha) bases[nb++] = (uint64_t)(uintptr_t)r->t.g.alpha;
    r->wide_in = resize_wide_in_ok(r->src_w, bases, nb) ? 1 : 0;
}

jxl_status resize_args(jxl_ctx* c, const CtxLink& l, const jxl_tensor_params* p, const jxl_resize_params* rz, const void* const in[3],
                       const void* alpha, void* out, ResizeArgs* r, TensorLayout* lay, bool check_out) {
    if (!out) return ctx_fail(c, JXL_ERR_INVALID_ARGUMENT, "tensor samples: null argument");
    const char* why = resize_check_params(p, rz);
    if (why) return ctx_fail(c, JXL_ERR_INVALID_ARGUMENT, why);
    return tensor_args(c, l, p, in, alpha, out, &r->t, lay, rz->out_height, rz->out_width, check_out);
}

}  // namespace jxl

using namespace jxl;

extern "C" {

jxl_status jxl_stage_tensor_resized(jxl_ctx* c, const void* const in[3], const void* alpha, const jxl_tensor_params* p,
                                    const jxl_resize_params* rz, void* out_device) {
    CtxLink l;
    jxl_status st = ctx_link(c, &l);
    if (st) return st;
    return resized_from_home(c, l, home_host(in, alpha), p, rz, out_device);
}

jxl_status jxl_planes_tensor_resized(jxl_ctx* c, const void* alpha, const jxl_tensor_params* p, const jxl_resize_params* rz,
                                     void* out_device) {
    CtxLink l;
    ImageHome m;
    jxl_status st = ctx_link(c, &l);
    if (st || (st = ctx_home_resident(c, alpha, &m))) return st;
    return resized_from_home(c, l, m, p, rz, out_device);
}

jxl_status jxl_canvas_tensor_resized(jxl_ctx* c, int32_t id, int32_t alpha_plane, const jxl_tensor_params* p, const jxl_resize_params* rz,
                                     void* out_device) {
    CtxLink l;
    ImageHome m;
    jxl_status st = ctx_link(c, &l);
    if (st || (st = tensor_home_set(c, id, alpha_plane, p, &m))) return st;
    return resized_from_home(c, l, m, p, rz, out_device);
}

// tests: the tile of the resized launches that follow, (0, 0) for the host's own choice again. A tile the kernel does not have
// is refused here; one whose LDS image does not fit a call's footprint is refused by that call
jxl_status jxl_debug_tensor_resize_tile(int32_t tw, int32_t th) {
    if (tw || th) {
        const bool known = (tw == 64 || tw == 32 || tw == 16 || tw == 8 || tw == 4 || tw == 2 || tw == 1) && (th == 4 || th == 2 || th == 1);
        if (!known) return JXL_ERR_INVALID_ARGUMENT;
    }
    g_force_tw = tw, g_force_th = th;
    return JXL_OK;
}

// measurements: the LDS skew of the resized launches that follow (on by default)
jxl_status jxl_debug_tensor_resize_skew(int32_t on) {
    g_skew = on != 0;
    return JXL_OK;
}

}  // extern "C"
