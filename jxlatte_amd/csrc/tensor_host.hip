// Host side of the tensor exit (k_tensor.hip): the three jxl_*_tensor_samples entries beside the PNG's three, each of them "resolve
// the image's home, then samples_from_home". The checks the PNG entries make are theirs (ctx_png_args, host.hip), the tensor's own
// pure checks are tensor_check.h's, those of a home image_home.h's -- in this file they get the tensor entries' words, for the
// resized and the batch entries too (tensor_host.h). What is left here is the question only the runtime can answer -- is
// out_device device memory of this context's device, and does its allocation hold the tensor -- and the launch. Nothing is queued
// before every check has passed; the stream is synchronised before return.
#include "tensor_host.h"

namespace jxl {

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
    const bool tone = ctx_tone_map_armed(c);
    const char* why = tensor_check_params(p, lay, tone);
    if (!why && (out_height || out_width)) {  // the tensor is out_height x out_width: its layout, bytes and alignment rule
        jxl_tensor_params q = *p;
        q.height = out_height, q.width = out_width;
        why = tensor_check_params(&q, lay, tone);
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
// the tensor entries' words for a home's refusal
jxl_status home_fail(jxl_ctx* c, HomeRefusal r, const ImageHome& m) {
    const char* why = r == HOME_UNKNOWN_SET       ? "canvas: unknown set"
                      : r == HOME_NO_SUCH_PLANES  ? "tensor samples: the set has no such planes"
                      : m.kind == HOME_RESIDENT   ? "tensor samples: the resident planes are three float planes of another size"
                                                  : "tensor samples: the parameters do not describe the set's planes";
    return ctx_fail(c, JXL_ERR_INVALID_ARGUMENT, why);
}
}  // namespace

jxl_status tensor_home_set(jxl_ctx* c, int32_t id, int32_t alpha_plane, const jxl_tensor_params* p, ImageHome* m) {
    *m = ctx_home_set(c, id, p ? p->color.n_planes : 0, alpha_plane, p && p->has_alpha);
    if (m->planes == HOME_UNKNOWN_SET) return home_fail(c, m->planes, *m);
    if (!p) return ctx_fail(c, JXL_ERR_INVALID_ARGUMENT, "tensor samples: null argument");
    return m->planes ? home_fail(c, m->planes, *m) : JXL_OK;
}

jxl_status tensor_home_fits(jxl_ctx* c, const ImageHome& m, const jxl_tensor_params* p) {
    const HomeRefusal r = home_describes(m, p->height, p->width, p->color.n_planes, p->color.in_is_int, p->alpha_is_int);
    return r ? home_fail(c, r, m) : JXL_OK;
}

jxl_status tensor_place(jxl_ctx* c, const ImageHome& m, const jxl_tensor_params* p, PngArgs* g, Staged* s) {
    const HomeUploads up = home_uploads(m);
    const size_t plane = (size_t)p->height * (size_t)p->width * 4;
    for (int i = 0; i < p->color.n_planes; i++)
        if (!(g->c.in[i] = up.color ? s->up(m.color[i], plane) : m.color[i])) return ctx_fail(c, JXL_ERR_OOM, "device allocation failed");
    if (tensor_alpha_read(p) && !(g->alpha = up.alpha ? s->up(m.alpha, plane) : m.alpha)) return ctx_fail(c, JXL_ERR_OOM, "device allocation failed");
    return JXL_OK;
}

namespace {

// the body of the three entries: tensor_args, the home's second half, the planes' places, the launch
jxl_status samples_from_home(jxl_ctx* c, const CtxLink& l, const ImageHome& m, const jxl_tensor_params* p, void* out, int max_workgroups) {
    TensorArgs t;
    TensorLayout lay;
    jxl_status st = tensor_args(c, l, p, m.in(), m.alpha, out, &t, &lay);
    if (st || (st = tensor_home_fits(c, m, p))) return st;
    Staged s;
    if ((st = tensor_place(c, m, p, &t.g, &s))) return st;
    launch_tensor_samples(t, l.stream, max_workgroups);
    TENSOR_HIP(c, hipStreamSynchronize(l.stream));
    TENSOR_HIP(c, hipGetLastError());
    return JXL_OK;
}

jxl_status stage_entry(jxl_ctx* c, const void* const in[3], const void* alpha, const jxl_tensor_params* p, void* out, int max_workgroups) {
    CtxLink l;
    jxl_status st = ctx_link(c, &l);
    if (st) return st;
    return samples_from_home(c, l, home_host(in, alpha), p, out, max_workgroups);
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
    ImageHome m;
    jxl_status st = ctx_link(c, &l);
    if (st || (st = ctx_home_resident(c, alpha, &m))) return st;
    return samples_from_home(c, l, m, p, out_device, 0);
}

jxl_status jxl_canvas_tensor_samples(jxl_ctx* c, int32_t id, int32_t alpha_plane, const jxl_tensor_params* p, void* out_device) {
    CtxLink l;
    ImageHome m;
    jxl_status st = ctx_link(c, &l);
    if (st || (st = tensor_home_set(c, id, alpha_plane, p, &m))) return st;
    return samples_from_home(c, l, m, p, out_device, 0);
}

}  // extern "C"
