// What jxl_canvas_patches and jxl_canvas_cast_planes refuse before anything is queued. Plain C++ (no device code, no context),
// so the checks can be compiled and run on their own (tools/native/canvas_patch_check.cpp).
#pragma once
#include <cstdint>

#include "../../include/jxlatte_amd.h"
#include "canvas_check.h"
#include "patch_compile.h"
#include "pfm_check.h"

namespace jxl {

// jxl_canvas_patches / jxl_canvas_patches_check: the set-level refusals, then patch_compile -- jxl_patch_bins' validation -- on
// the sizes and plane types the sets give. frame: the frame set's shape; ref[k]: slot k's, or null for reference[k] == null;
// aliased: the frame set is one of the reference sets (the entries tell by id, the check entry by the shape object).
// JXL_OK and *out, or the status with the reason in *why and the offending position in *first_bad (-1: none).
inline jxl_status canvas_patches_check(const jxl_patch_desc* d, const jxl_canvas_shape* frame, int32_t colors_resident,
                                       const jxl_canvas_shape* const* ref, bool aliased, PatchStage* out, const char** why,
                                       int32_t* first_bad) {
    const char* dummy;
    int32_t dummy_bad;
    if (!why) why = &dummy;
    if (!first_bad) first_bad = &dummy_bad;
    *first_bad = -1;
    if (!d || !frame || !ref || !out) return *why = "canvas patches: null argument", JXL_ERR_INVALID_ARGUMENT;
    const int64_t n_chan = (int64_t)d->n_color + d->n_extra;
    if (frame->n != n_chan) return *why = "canvas patches: the frame set holds one plane per channel", JXL_ERR_INVALID_ARGUMENT;
    for (int k = 0; k < 4; k++)
        if (ref[k] && ref[k]->n != n_chan) return *why = "canvas patches: a reference set holds one plane per channel", JXL_ERR_INVALID_ARGUMENT;
    if (n_chan > JXL_CANVAS_MAX_PLANES) return *why = "canvas patches: more than 16 planes", JXL_ERR_UNSUPPORTED;
    if (!canvas_shape_ok(frame)) return *why = "canvas patches: bad plane set", JXL_ERR_INVALID_ARGUMENT;
    for (int k = 0; k < 4; k++)
        if (ref[k] && !canvas_shape_ok(ref[k])) return *why = "canvas patches: bad plane set", JXL_ERR_INVALID_ARGUMENT;
    if (colors_resident && d->n_color != 3) return *why = "patches: the resident planes are three colour planes", JXL_ERR_INVALID_ARGUMENT;
    if (aliased) return *why = "canvas patches: the frame set is a reference set", JXL_ERR_INVALID_ARGUMENT;
    jxl_patch_desc q = *d;
    int32_t frame_type[JXL_CANVAS_MAX_PLANES], ref_type[4 * JXL_CANVAS_MAX_PLANES];
    for (int ch = 0; ch < n_chan; ch++) frame_type[ch] = colors_resident && ch < 3 ? JXL_PLANE_FLOAT : frame->types[ch];
    for (int k = 0; k < 4; k++) {
        q.ref_h[k] = ref[k] ? ref[k]->h : 0;
        q.ref_w[k] = ref[k] ? ref[k]->w : 0;
        for (int ch = 0; ch < n_chan; ch++) ref_type[k * n_chan + ch] = ref[k] ? ref[k]->types[ch] : -1;
    }
    return patch_compile(&q, frame->h, frame->w, frame_type, ref_type, out, why, first_bad);
}

// jxl_canvas_cast_planes: shape_of(set id) gives a set's shape or null for an unknown id. JXL_OK and scale[i] = 1f / max for the
// items to cast (0: the plane is float already and is skipped), or JXL_ERR_INVALID_ARGUMENT with the reason in *why. The items are
// looked at in order; per item: the set, the plane, whether it was named before, then -- for an int32 plane only, as
// jxl_canvas_cast -- its depth.
constexpr int32_t kCanvasMaxCasts = 5 * JXL_CANVAS_MAX_PLANES;
template <typename ShapeOf>
inline jxl_status canvas_cast_list_check(int32_t n, const jxl_canvas_cast_item* items, ShapeOf shape_of, float* scale, const char** why) {
    const char* dummy;
    if (!why) why = &dummy;
    if (n < 0 || (n > 0 && (!items || !scale))) return *why = "canvas cast: bad arguments", JXL_ERR_INVALID_ARGUMENT;
    if (n > kCanvasMaxCasts) return *why = "canvas cast: more than 80 planes in one call", JXL_ERR_INVALID_ARGUMENT;
    for (int32_t i = 0; i < n; i++) {
        const jxl_canvas_cast_item& it = items[i];
        const jxl_canvas_shape* s = shape_of(it.set);
        if (!s) return *why = "canvas: unknown set", JXL_ERR_INVALID_ARGUMENT;
        if (it.plane < 0 || it.plane >= s->n) return *why = "canvas cast: bad plane", JXL_ERR_INVALID_ARGUMENT;
        for (int32_t j = 0; j < i; j++)
            if (items[j].set == it.set && items[j].plane == it.plane) return *why = "canvas cast: a plane is named twice", JXL_ERR_INVALID_ARGUMENT;
        scale[i] = 0.0f;
        if (s->types[it.plane] == JXL_PLANE_FLOAT) continue;  // ImageBuffer.java:100-101
        const int32_t max = pfm_depth_max(it.depth);
        if (max < 1) return *why = "invalid Max Value", JXL_ERR_INVALID_ARGUMENT;  // ImageBuffer.java:115-116
        scale[i] = 1.0f / (float)max;                                              // ImageBuffer.java:119
    }
    return JXL_OK;
}

}  // namespace jxl
