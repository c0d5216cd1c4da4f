// Host side of the tensor exit (k_tensor.hip): the three jxl_*_tensor_samples entries beside the PNG's three. The checks the PNG
// entries make are theirs (ctx_png_args, host.hip), the tensor's own pure checks are tensor_check.h's; what is left here is the
// question only the runtime can answer -- is out_device device memory of this context's device, and does its allocation hold the
// tensor -- and the launch. Nothing is queued before every check has passed; the stream is synchronised before return.
#include "tensor_host.h"

namespace jxl {

#define TS_HIP(c, expr)                                                                                                        \
    do {                                                                                                                      \
        hipError_t e_ = (expr);                                                                                               \
        if (e_ != hipSuccess) return ctx_fail(c, e_ == hipErrorOutOfMemory ? JXL_ERR_OOM : JXL_ERR_DEVICE, hipGetErrorString(e_)); \
    } while (0)

jxl_status tensor_out_check(jxl_ctx* c, const CtxLink& l, void* out, uint64_t bytes) {
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, out) != hipSuccess) {
        (void)hipGetLastError();  // (an address the runtime does not know: its error is not the stream's)
        return ctx_fail(c, JXL_ERR_INVALID_ARGUMENT, "tensor samples: out_device is not device memory");
    }
    if (at.type != hipMemoryTypeDevice || at.device != l.device)
        return ctx_fail(c, JXL_ERR_INVALID_ARGUMENT, "tensor samples: out_device is not device memory of the context's device");
    hipDeviceptr_t base = nullptr;
    size_t range = 0;
    if (hipMemGetAddressRange(&base, &range, (hipDeviceptr_t)out) != hipSuccess) {
        (void)hipGetLastError();
        return ctx_fail(c, JXL_ERR_INVALID_ARGUMENT, "tensor samples: out_device belongs to no allocation");
    }
    if (!tensor_extent_ok((uint64_t)(uintptr_t)base, (uint64_t)range, (uint64_t)(uintptr_t)out, bytes))
        return ctx_fail(c, JXL_ERR_INVALID_ARGUMENT, "tensor samples: the allocation of out_device ends before the tensor does");
    return JXL_OK;
}

jxl_status tensor_args(jxl_ctx* c, const CtxLink& l, const jxl_tensor_params* p, const void* const in[3], const void* alpha, void* out,
                       TensorArgs* t, TensorLayout* lay, int32_t out_height, int32_t out_width, bool check_out) {
    if (!out) return ctx_fail(c, JXL_ERR_INVALID_ARGUMENT, "tensor samples: null argument");
    const char* why = tensor_check_params(p, lay);
    if (!why && (out_height || out_width)) {  // the tensor is out_height x out_width: its layout, bytes and alignment rule
        jxl_tensor_params q = *p;
        q.height = out_height, q.width = out_width;
        why = tensor_check_params(&q, lay);
    }
    if (why) return ctx_fail(c, JXL_ERR_INVALID_ARGUMENT, why);
    jxl_png_params g;
    g.color = p->color;
    g.height = p->height, g.width = p->width;
    g.has_alpha = p->has_alpha, g.premultiplied = p->premultiplied;
    g.bit_depth = 8, g.big_endian = 0;
    g.alpha_is_int = p->alpha_is_int, g.alpha_tagged_depth = p->alpha_tagged_depth, g.color_tagged_depth = p->color_tagged_depth;
    int n_color = 0;
    jxl_status st = ctx_png_args(c, &g, in, alpha, out, &t->g, &n_color);
    if (st) return st;
    if (check_out && (st = tensor_out_check(c, l, out, lay->bytes))) return st;
    t->dtype = p->dtype, t->layout = p->layout;
    t->n_out = lay->n_out;
    t->use_norm = p->use_norm ? 1 : 0;
    for (int i = 0; i < 4; i++) t->mean[i] = p->mean[i], t->inv_std[i] = p->inv_std[i];
    t->wide = tensor_wide_ok((uint64_t)(uintptr_t)out, p->layout, *lay) ? 1 : 0;
    t->out = out;
    return JXL_OK;
}

namespace {

bool alpha_read(const jxl_tensor_params* p) { return tensor_alpha_read(p); }

jxl_status tensor_run(jxl_ctx* c, const CtxLink& l, const TensorArgs& t, int max_workgroups) {
    launch_tensor_samples(t, l.stream, max_workgroups);
    TS_HIP(c, hipStreamSynchronize(l.stream));
    TS_HIP(c, hipGetLastError());
    return JXL_OK;
}

jxl_status stage_entry(jxl_ctx* c, const void* const in[3], const void* alpha, const jxl_tensor_params* p, void* out, int max_workgroups) {
    CtxLink l;
    jxl_status st = ctx_link(c, &l);
    if (st) return st;
    TensorArgs t;
    TensorLayout lay;
    if ((st = tensor_args(c, l, p, in, alpha, out, &t, &lay))) return st;
    Staged s;
    const size_t plane = (size_t)lay.pixels * 4;
    for (int i = 0; i < p->color.n_planes; i++)
        if (!(t.g.c.in[i] = s.up(in[i], plane))) return ctx_fail(c, JXL_ERR_OOM, "device allocation failed");
    if (alpha_read(p) && !(t.g.alpha = s.up(alpha, plane))) return ctx_fail(c, JXL_ERR_OOM, "device allocation failed");
    return tensor_run(c, l, t, max_workgroups);
}

}  // namespace
}  // namespace jxl

using namespace jxl;

extern "C" {

jxl_status jxl_stage_tensor_samples(jxl_ctx* c, const void* const in[3], const void* alpha, const jxl_tensor_params* p, void* out_device) {
    return stage_entry(c, in, alpha, p, out_device, 0);
}

// tests: jxl_stage_tensor_samples on a grid of at most max_workgroups workgroups (the grid-stride loop at a small size)
jxl_status jxl_debug_tensor_samples_grid(jxl_ctx* c, const void* const in[3], const void* alpha, const jxl_tensor_params* p, void* out_device,
                                         int32_t max_workgroups) {
    if (max_workgroups < 1) return ctx_fail(c, JXL_ERR_INVALID_ARGUMENT, "tensor samples: bad grid bound");
    return stage_entry(c, in, alpha, p, out_device, max_workgroups);
}

jxl_status jxl_planes_tensor_samples(jxl_ctx* c, const void* alpha, const jxl_tensor_params* p, void* out_device) {
    CtxLink l;
    jxl_status st = ctx_link(c, &l);
    if (st) return st;
    int h = 0, w = 0;
    float* rp[3];
    if ((st = ctx_planes_get(c, &h, &w, rp))) return st;
    const void* in[3] = {rp[0], rp[1], rp[2]};
    TensorArgs t;
    TensorLayout lay;
    if ((st = tensor_args(c, l, p, in, alpha, out_device, &t, &lay))) return st;
    if (p->color.n_planes != 3 || p->color.in_is_int || p->height != h || p->width != w)
        return ctx_fail(c, JXL_ERR_INVALID_ARGUMENT, "tensor samples: the resident planes are three float planes of another size");
    for (int i = 0; i < 3; i++) t.g.c.in[i] = in[i];
    Staged s;
    if (alpha_read(p) && !(t.g.alpha = s.up(alpha, (size_t)lay.pixels * 4))) return ctx_fail(c, JXL_ERR_OOM, "device allocation failed");
    return tensor_run(c, l, t, 0);
}

jxl_status jxl_canvas_tensor_samples(jxl_ctx* c, int32_t id, int32_t alpha_plane, const jxl_tensor_params* p, void* out_device) {
    CtxLink l;
    jxl_status st = ctx_link(c, &l);
    if (st) return st;
    CanvasView v;
    if (!canvas_view(*l.canvas, id, &v)) return ctx_fail(c, JXL_ERR_INVALID_ARGUMENT, "canvas: unknown set");
    if (!p) return ctx_fail(c, JXL_ERR_INVALID_ARGUMENT, "tensor samples: null argument");
    const int nc = p->color.n_planes;
    if ((nc != 1 && nc != 3) || nc > v.n || alpha_plane < -1 || alpha_plane >= v.n || (p->has_alpha != 0) != (alpha_plane >= 0))
        return ctx_fail(c, JXL_ERR_INVALID_ARGUMENT, "tensor samples: the set has no such planes");
    const void* in[3] = {nullptr, nullptr, nullptr};
    for (int i = 0; i < nc; i++) in[i] = v.plane[i];
    const void* alpha = alpha_plane >= 0 ? v.plane[alpha_plane] : nullptr;
    TensorArgs t;
    TensorLayout lay;
    if ((st = tensor_args(c, l, p, in, alpha, out_device, &t, &lay))) return st;
    bool tags = p->height == v.h && p->width == v.w;
    for (int i = 0; i < nc; i++) tags = tags && (p->color.in_is_int != 0) == (v.type[i] == JXL_PLANE_INT32);
    if (alpha_plane >= 0) tags = tags && (p->alpha_is_int != 0) == (v.type[alpha_plane] == JXL_PLANE_INT32);
    if (!tags) return ctx_fail(c, JXL_ERR_INVALID_ARGUMENT, "tensor samples: the parameters do not describe the set's planes");
    for (int i = 0; i < nc; i++) t.g.c.in[i] = in[i];
    if (alpha_read(p)) t.g.alpha = alpha;
    return tensor_run(c, l, t, 0);
}

}  // extern "C"
