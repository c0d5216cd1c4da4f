// Host side of noise on a window of a frame (k_noise_window.hip): jxl_planes_noise_at on the resident planes and
// jxl_stage_noise_window on host planes. The arguments are checked by noise_window_check.h before anything is allocated; the
// raw noise of the apron lives in scratch that is freed on return.
#include "noise_window.h"
#include "tensor_host.h"

namespace jxl {
namespace {

#define NW_HIP(c, expr)                                                                                                        \
    do {                                                                                                                      \
        hipError_t e_ = (expr);                                                                                               \
        if (e_ != hipSuccess) return ctx_fail(c, e_ == hipErrorOutOfMemory ? JXL_ERR_OOM : JXL_ERR_DEVICE, hipGetErrorString(e_)); \
    } while (0)

// the apron's scratch and both launches on device planes of the window's size; the stream is left running
jxl_status noise_window_run(jxl_ctx* c, const CtxLink& l, const NoiseWindowPlan& plan, uint64_t seed0, const float lut[8], float bcx, float bcb,
                            float* const planes[3], Staged* s) {
    float* apron[3];
    for (int i = 0; i < 3; i++)
        if (!(apron[i] = (float*)s->alloc(sizeof(float) * (size_t)plan.apron_floats))) return ctx_fail(c, JXL_ERR_OOM, "device allocation failed (noise apron)");
    launch_noise_window(plan, seed0, apron, planes, lut, bcx, bcb, l.stream);
    NW_HIP(c, hipGetLastError());
    return JXL_OK;
}

}  // namespace
}  // namespace jxl

using namespace jxl;

extern "C" {

jxl_status jxl_planes_noise_at(jxl_ctx* c, int32_t group_dim, uint64_t seed0, const float lut[8], float base_corr_x, float base_corr_b,
                               int32_t frame_h, int32_t frame_w, int32_t y0, int32_t x0) {
    CtxLink l;
    jxl_status st = ctx_link(c, &l);
    if (st) return st;
    int h = 0, w = 0;
    float* planes[3];
    if ((st = ctx_planes_get(c, &h, &w, planes))) return st;
    NoiseWindowPlan plan;
    const char* why = noise_window_check(group_dim, lut, frame_h, frame_w, y0, x0, h, w, &plan);
    if (why) return ctx_fail(c, JXL_ERR_INVALID_ARGUMENT, why);
    Staged s;
    if ((st = noise_window_run(c, l, plan, seed0, lut, base_corr_x, base_corr_b, planes, &s))) return st;
    NW_HIP(c, hipStreamSynchronize(l.stream));  // the apron is freed on return
    return JXL_OK;
}

jxl_status jxl_stage_noise_window(jxl_ctx* c, float* const planes[3], int32_t height, int32_t width, int32_t group_dim, uint64_t seed0,
                                  const float lut[8], float base_corr_x, float base_corr_b, int32_t frame_h, int32_t frame_w, int32_t y0,
                                  int32_t x0) {
    CtxLink l;
    jxl_status st = ctx_link(c, &l);
    if (st) return st;
    if (!planes || !planes[0] || !planes[1] || !planes[2]) return ctx_fail(c, JXL_ERR_INVALID_ARGUMENT, "noise window: null plane");
    NoiseWindowPlan plan;
    const char* why = noise_window_check(group_dim, lut, frame_h, frame_w, y0, x0, height, width, &plan);
    if (why) return ctx_fail(c, JXL_ERR_INVALID_ARGUMENT, why);
    Staged s;
    const size_t bytes = sizeof(float) * (size_t)plan.window_floats;
    float* d[3];
    for (int i = 0; i < 3; i++) {
        if (!(d[i] = (float*)s.alloc(bytes))) return ctx_fail(c, JXL_ERR_OOM, "device allocation failed");
        NW_HIP(c, hipMemcpy(d[i], planes[i], bytes, hipMemcpyHostToDevice));
    }
    if ((st = noise_window_run(c, l, plan, seed0, lut, base_corr_x, base_corr_b, d, &s))) return st;
    NW_HIP(c, hipStreamSynchronize(l.stream));
    for (int i = 0; i < 3; i++) NW_HIP(c, hipMemcpy(planes[i], d[i], bytes, hipMemcpyDeviceToHost));
    return JXL_OK;
}

}  // extern "C"
