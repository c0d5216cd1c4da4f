// Which inner blend function blendBuffers' switch reaches (JXLCodestreamDecoder.java:285-413, 493-512), and which planes it reads.
// Plain C++ (no device code, no context): shared by k_blend's launcher (k_post.hip), the patch stage (patch_compile.h) and the
// checks of canvas_check.h.
#pragma once
#include "../../include/jxlatte_amd.h"

namespace jxl {

// the inner blend functions (k_blend's switch); blend_op maps (mode, flags, is_int) to one; -1 illegal mode, -2 int samples on a
// float-only function
enum BlendOp { OP_COPY_FRAME, OP_COPY_REF, OP_ADD_I, OP_ADD_F, OP_MULT, OP_BLEND, OP_MULADD };

inline int blend_op(int mode, unsigned flags, int is_int) {
    const bool is_alpha = flags & JXL_BLEND_FLAG_IS_ALPHA, has_extra = flags & JXL_BLEND_FLAG_HAS_EXTRA;
    int op;
    switch (mode) {
        case JXL_BLEND_REPLACE: op = OP_COPY_FRAME; break;
        case JXL_BLEND_ADD: op = is_int ? OP_ADD_I : OP_ADD_F; break;
        case JXL_BLEND_MULT: op = OP_MULT; break;
        case JXL_BLEND_BLEND: op = has_extra ? OP_BLEND : (is_int ? OP_ADD_I : OP_ADD_F); break;  // :346-349
        case JXL_BLEND_MULADD: op = !has_extra ? (is_int ? OP_ADD_I : OP_ADD_F) : is_alpha ? OP_COPY_REF : OP_MULADD; break;
        default: return -1;  // "Illegal blend mode"
    }
    if (is_int && op != OP_COPY_FRAME && op != OP_COPY_REF && op != OP_ADD_I) return -2;
    return op;
}

inline bool blend_needs(int op, bool* frame, bool* ref, bool* frame_alpha, bool* ref_alpha, bool is_alpha) {
    *frame = op != OP_COPY_REF;
    *ref = op != OP_COPY_FRAME;
    *frame_alpha = (op == OP_BLEND && !is_alpha) || op == OP_MULADD;
    *ref_alpha = op == OP_BLEND && !is_alpha;
    return true;
}

}  // namespace jxl
