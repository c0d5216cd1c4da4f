// Host side of the LF image at 1:8 (k_lf_image.hip): jxl_planes_from_lf and jxl_stage_lf_image. The descriptor is checked by
// lf_image_check.h before anything is allocated; the group table and every LF group's integers go up in ONE transfer; one launch.
#include "lf_image.h"
#include "lf_image_check.h"
#include "tensor_host.h"

#include <cstring>

namespace jxl {
namespace {

#define LFI_HIP(c, expr)                                                                                                       \
    do {                                                                                                                      \
        hipError_t e_ = (expr);                                                                                               \
        if (e_ != hipSuccess) return ctx_fail(c, e_ == hipErrorOutOfMemory ? JXL_ERR_OOM : JXL_ERR_DEVICE, hipGetErrorString(e_)); \
    } while (0)

// the checks, the one block, the launch into out[3] (device planes of cells_h x cells_w floats); the stream is left running
jxl_status lf_image_run(jxl_ctx* c, const CtxLink& l, const jxl_lf_image_desc* d, const LfImagePlan& plan, float* const out[3], Staged* s) {
    const size_t table = sizeof(LfImageGroup) * (size_t)d->n_groups, block = table + 4 * (size_t)plan.total_ints;
    std::vector<char> pack(block);
    for (int p = 0; p < d->n_groups; p++) {
        const jxl_lfquant_desc& g = d->groups[plan.order[(size_t)p]];
        LfImageGroup t;
        std::memset(&t, 0, sizeof t);
        for (int i = 0; i < 3; i++) {
            t.q_off[i] = plan.q_off[(size_t)p * 3 + i];
            t.sd[i] = g.scaled_dequant[i] / (float)(1 << g.extra_precision);  // LFCoefficients.java:69
            t.sd_gap[i] = g.scaled_dequant[i];
            std::memcpy(pack.data() + table + 4 * (size_t)t.q_off[i], g.lf_quant[i], 4 * (size_t)g.cells_h * g.cells_w);
        }
        t.H = g.cells_h;
        t.W = g.cells_w;
        // SPEC: -128, not -127 (LFCoefficients.java:80-82); launch_lf_dequant's expressions
        t.kX = d->base_corr_x + ((float)g.x_factor_lf - 128.0f) / (float)d->color_factor;
        t.kB = d->base_corr_b + ((float)g.b_factor_lf - 128.0f) / (float)d->color_factor;
        t.smooth = g.adaptive_smoothing ? 1 : 0;
        std::memcpy(pack.data() + sizeof(LfImageGroup) * (size_t)p, &t, sizeof t);
    }
    char* dev = (char*)s->alloc(block);
    if (!dev) return ctx_fail(c, JXL_ERR_OOM, "device allocation failed");
    LFI_HIP(c, hipMemcpy(dev, pack.data(), block, hipMemcpyHostToDevice));
    LfImageArgs a;
    std::memset(&a, 0, sizeof a);
    a.groups = (const LfImageGroup*)dev;
    a.ints = (const int32_t*)(dev + table);
    for (int i = 0; i < 3; i++) a.out[i] = out[i];
    a.H = d->cells_h;
    a.W = d->cells_w;
    a.gcols = plan.gcols;
    a.xyb = d->xyb ? 1 : 0;
    if (a.xyb) a.xybp = ctx_make_xyb(d->opsin_matrix, d->opsin_bias, d->cbrt_opsin_bias, d->intensity_target);
    launch_lf_image(a, l.stream);
    LFI_HIP(c, hipGetLastError());
    return JXL_OK;
}

}  // namespace
}  // namespace jxl

using namespace jxl;

extern "C" {

jxl_status jxl_planes_from_lf(jxl_ctx* c, const jxl_lf_image_desc* d) {
    CtxLink l;
    jxl_status st = ctx_link(c, &l);
    if (st) return st;
    LfImagePlan plan;
    const char* why = lf_image_check(d, nullptr, false, &plan);
    if (why) return ctx_fail(c, JXL_ERR_INVALID_ARGUMENT, why);
    LFI_HIP(c, hipStreamSynchronize(l.stream));  // (the planes may be replaced: nothing queued still reads them)
    float* out[3];
    if ((st = ctx_planes_set(c, d->cells_h, d->cells_w, out))) return st;
    Staged s;
    if ((st = lf_image_run(c, l, d, plan, out, &s))) return st;
    LFI_HIP(c, hipStreamSynchronize(l.stream));  // the block is freed on return
    return JXL_OK;
}

jxl_status jxl_stage_lf_image(jxl_ctx* c, const jxl_lf_image_desc* d, float* const out[3]) {
    CtxLink l;
    jxl_status st = ctx_link(c, &l);
    if (st) return st;
    LfImagePlan plan;
    const char* why = lf_image_check(d, out, true, &plan);
    if (why) return ctx_fail(c, JXL_ERR_INVALID_ARGUMENT, why);
    Staged s;
    const size_t plane = 4 * (size_t)d->cells_h * d->cells_w;
    float* dout[3];
    for (int i = 0; i < 3; i++)
        if (!(dout[i] = (float*)s.alloc(plane))) return ctx_fail(c, JXL_ERR_OOM, "device allocation failed");
    if ((st = lf_image_run(c, l, d, plan, dout, &s))) return st;
    LFI_HIP(c, hipStreamSynchronize(l.stream));
    for (int i = 0; i < 3; i++) LFI_HIP(c, hipMemcpy(out[i], dout[i], plane, hipMemcpyDeviceToHost));
    return JXL_OK;
}

}  // extern "C"
