// jxl_modular_planes_desc: what jxl_canvas_from_modular and jxl_canvas_from_modular_up refuse. Plain C++ (no device code, no
// context), so the checks can be compiled and run on their own (tools/native/modplanes_check.cpp, modplanes_up_check.cpp).
#pragma once
#include <cstdint>

#include "../../include/jxlatte_amd.h"

namespace jxl {

struct ModPlaneShape { int32_t h, w; };  // one result channel of the Modular context

// JXL_OK: every plane of `d` can be read from the result list out[0 .. n_out); else the status, with what is wrong in *why.
// ran: a plan has run since jxl_modular_begin
inline jxl_status modplanes_check(const jxl_modular_planes_desc* d, const ModPlaneShape* out, int32_t n_out, bool ran, const char** why) {
    const char* dummy;
    if (!why) why = &dummy;
    if (!d || (n_out > 0 && !out)) return *why = "modular planes: null argument", JXL_ERR_INVALID_ARGUMENT;
    if (!ran) return *why = "modular planes: no plan has run", JXL_ERR_STATE;
    if (d->n_planes > JXL_CANVAS_MAX_PLANES) return *why = "canvas: more than 16 planes", JXL_ERR_UNSUPPORTED;
    if (d->n_planes < 1) return *why = "modular planes: no planes", JXL_ERR_INVALID_ARGUMENT;
    if (d->height < 1 || d->width < 1) return *why = "modular planes: bad size", JXL_ERR_INVALID_ARGUMENT;
    for (int i = 0; i < d->n_planes; i++) {
        const jxl_modular_plane& p = d->plane[i];
        if (p.type != JXL_PLANE_FLOAT && p.type != JXL_PLANE_INT32) return *why = "canvas: plane type", JXL_ERR_INVALID_ARGUMENT;
        if (p.channel < 0 || p.channel >= n_out) return *why = "modular planes: channel index out of range", JXL_ERR_INVALID_ARGUMENT;
        const ModPlaneShape& a = out[p.channel];
        if (a.h < d->height || a.w < d->width) return *why = "modular planes: a channel is smaller than the bounds", JXL_ERR_INVALID_ARGUMENT;
        if (p.add_channel == -1) continue;
        if (p.type == JXL_PLANE_INT32) return *why = "modular planes: an int32 plane takes no second channel", JXL_ERR_INVALID_ARGUMENT;
        if (p.add_channel < 0 || p.add_channel >= n_out) return *why = "modular planes: channel index out of range", JXL_ERR_INVALID_ARGUMENT;
        const ModPlaneShape& b = out[p.add_channel];
        if (b.h != a.h || b.w != a.w) return *why = "modular planes: the added channel has another size", JXL_ERR_INVALID_ARGUMENT;
    }
    return JXL_OK;
}

// jxl_canvas_from_modular_up: everything above, then what the upsampling adds. have_weights: the weights pointer is not null
inline jxl_status modplanes_up_check(const jxl_modular_planes_desc* d, const ModPlaneShape* out, int32_t n_out, bool ran, int32_t k,
                                     bool have_weights, const char** why) {
    const char* dummy;
    if (!why) why = &dummy;
    const jxl_status st = modplanes_check(d, out, n_out, ran, why);
    if (st) return st;
    if (k != 2 && k != 4 && k != 8) return *why = "modular planes: upsampling factor other than 2, 4 or 8", JXL_ERR_INVALID_ARGUMENT;
    if (!have_weights) return *why = "modular planes: null weights", JXL_ERR_INVALID_ARGUMENT;
    for (int i = 0; i < d->n_planes; i++)  // the reference casts before it upsamples (Frame.java:228)
        if (d->plane[i].type != JXL_PLANE_FLOAT) return *why = "modular planes: an upsampled plane is a float plane", JXL_ERR_INVALID_ARGUMENT;
    if ((int64_t)d->height * k > INT32_MAX || (int64_t)d->width * k > INT32_MAX)
        return *why = "modular planes: the upsampled size is beyond what a set holds", JXL_ERR_INVALID_ARGUMENT;
    return JXL_OK;
}

}  // namespace jxl
