// jxl_canvas_blend_desc: what jxl_canvas_blend refuses, and per channel the inner blend function and the planes it reads. Plain
// C++ (no device code, no context), so the checks can be compiled and run on their own.
#pragma once
#include <cstdint>

#include "../../include/jxlatte_amd.h"
#include "blend_ops.h"

namespace jxl {

struct CanvasChanOp {
    int op;                                     // BlendOp
    bool frame, ref, frame_alpha, ref_alpha;    // the planes the function reads (blend_needs)
};

inline bool canvas_shape_ok(const jxl_canvas_shape* s) {
    if (!s || s->n < 1 || s->n > JXL_CANVAS_MAX_PLANES || s->h < 1 || s->w < 1) return false;
    for (int i = 0; i < s->n; i++)
        if (s->types[i] != JXL_PLANE_FLOAT && s->types[i] != JXL_PLANE_INT32) return false;
    return true;
}

// jxl_canvas_take_planes: set is null for an unknown id; planes_h <= 0: the context has no resident planes
inline jxl_status canvas_take_check(const jxl_canvas_shape* set, int32_t planes_h, int32_t planes_w, const char** why) {
    const char* dummy;
    if (!why) why = &dummy;
    if (!set) return *why = "canvas: unknown set", JXL_ERR_INVALID_ARGUMENT;
    if (set->n < 3) return *why = "canvas: the set has fewer than three planes", JXL_ERR_INVALID_ARGUMENT;
    if (planes_h <= 0 || planes_w <= 0) return *why = "no resident planes", JXL_ERR_STATE;
    if (set->h != planes_h || set->w != planes_w) return *why = "canvas: the resident planes have another size than the set", JXL_ERR_INVALID_ARGUMENT;
    return JXL_OK;
}

// JXL_OK and ops[0 .. n_chan), or the status with the reason in *why
inline jxl_status canvas_blend_check(const jxl_canvas_blend_desc* d, const jxl_canvas_shape* canvas, const jxl_canvas_shape* frame,
                                     const jxl_canvas_shape* ref, CanvasChanOp* ops, const char** why) {
    if (!d || !canvas || !frame) return *why = "canvas blend: null argument", JXL_ERR_INVALID_ARGUMENT;
    if (canvas->n > JXL_CANVAS_MAX_PLANES || frame->n > JXL_CANVAS_MAX_PLANES || (ref && ref->n > JXL_CANVAS_MAX_PLANES))
        return *why = "canvas blend: more than 16 planes", JXL_ERR_UNSUPPORTED;
    if (!canvas_shape_ok(canvas) || !canvas_shape_ok(frame) || (ref && !canvas_shape_ok(ref)))
        return *why = "canvas blend: bad plane set", JXL_ERR_INVALID_ARGUMENT;
    if (d->canvas < 0 || d->frame < 0 || d->ref < -1 || d->canvas == d->frame || d->ref == d->frame)
        return *why = "canvas blend: bad set ids", JXL_ERR_INVALID_ARGUMENT;
    if ((d->ref == -1) != (ref == nullptr)) return *why = "canvas blend: reference id and reference shape disagree", JXL_ERR_INVALID_ARGUMENT;
    if (d->n_chan != canvas->n) return *why = "canvas blend: one entry per canvas channel", JXL_ERR_INVALID_ARGUMENT;
    const bool aliased = d->ref == d->canvas;
    if (aliased && (ref->n != canvas->n || ref->h != canvas->h || ref->w != canvas->w))
        return *why = "canvas blend: the reference is the canvas but its shape is not", JXL_ERR_INVALID_ARGUMENT;
    const jxl_blend_rect& r = d->rect;
    // the rectangle must lie inside every plane that is touched (Java would throw ArrayIndexOutOfBounds)
    auto inside = [&](int64_t y, int64_t x, const jxl_canvas_shape* s) {
        return r.h >= 0 && r.w >= 0 && y >= 0 && x >= 0 && y + r.h <= s->h && x + r.w <= s->w;
    };
    if (!inside(r.canvas_y, r.canvas_x, canvas)) return *why = "blend: rectangle outside a plane", JXL_ERR_INVALID_ARGUMENT;
    for (int c = 0; c < d->n_chan; c++) {
        const jxl_canvas_blend_chan& k = d->chan[c];
        if (k.frame_plane < 0 || k.frame_plane >= frame->n) return *why = "canvas blend: frame plane out of range", JXL_ERR_INVALID_ARGUMENT;
        const int ft = frame->types[k.frame_plane];
        const int op = blend_op(k.mode, k.flags, ft == JXL_PLANE_INT32);
        if (op == -1) return *why = "Illegal blend mode", JXL_ERR_INVALID_BITSTREAM;  // JXLCodestreamDecoder.java:510-511
        if (op == -2) return *why = "blend: this mode works on float samples", JXL_ERR_INVALID_ARGUMENT;
        CanvasChanOp o{op, false, false, false, false};
        blend_needs(op, &o.frame, &o.ref, &o.frame_alpha, &o.ref_alpha, (k.flags & JXL_BLEND_FLAG_IS_ALPHA) != 0);
        if ((o.ref || o.ref_alpha) && !ref) return *why = "blend: a plane this mode reads is NULL", JXL_ERR_INVALID_ARGUMENT;
        // blendBuffers has made the three planes of a channel one type before its switch (:433-436, :461-465); the copy of
        // REPLACE has only canvas and frame (:433-439)
        if (canvas->types[c] != ft) return *why = "canvas blend: canvas and frame plane differ in type", JXL_ERR_INVALID_ARGUMENT;
        if (o.ref && (c >= ref->n || ref->types[c] != ft)) return *why = "canvas blend: reference and frame plane differ in type", JXL_ERR_INVALID_ARGUMENT;
        if (o.frame_alpha && (k.frame_alpha < 0 || k.frame_alpha >= frame->n || frame->types[k.frame_alpha] != JXL_PLANE_FLOAT))
            return *why = "canvas blend: the frame's alpha plane is missing or not float", JXL_ERR_INVALID_ARGUMENT;
        if (o.ref_alpha && (k.ref_alpha < 0 || k.ref_alpha >= ref->n || ref->types[k.ref_alpha] != JXL_PLANE_FLOAT))
            return *why = "canvas blend: the reference's alpha plane is missing or not float", JXL_ERR_INVALID_ARGUMENT;
        const bool copy_ref = o.ref && !o.frame;  // blendMulAdd's alpha case indexes ref with frameOffset (:390)
        if ((o.frame || o.frame_alpha) && !inside(r.frame_y, r.frame_x, frame)) return *why = "blend: rectangle outside a plane", JXL_ERR_INVALID_ARGUMENT;
        if ((o.ref || o.ref_alpha) && !inside(copy_ref ? r.frame_y : r.ref_y, copy_ref ? r.frame_x : r.ref_x, ref))
            return *why = "blend: rectangle outside a plane", JXL_ERR_INVALID_ARGUMENT;
        // in place: a lane may read the canvas only where it writes it
        if (aliased && (o.ref || o.ref_alpha)) {
            const int32_t ry = copy_ref ? r.frame_y : r.ref_y, rx = copy_ref ? r.frame_x : r.ref_x;
            if (ry != r.canvas_y || rx != r.canvas_x)
                return *why = "canvas blend: the reference is the canvas and is read away from the pixel that is written", JXL_ERR_UNSUPPORTED;
        }
        if (ops) ops[c] = o;
    }
    return JXL_OK;
}

}  // namespace jxl
