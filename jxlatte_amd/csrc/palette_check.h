// jxl_palette_desc: what jxl_stage_palette refuses (ModularStream.java:327-378). Plain C++ (no device code, no context), so it
// can be compiled and run on its own (tools/native/palette_check.cpp). A descriptor that passes makes every read of the
// kernels of k_palette.hip safe without a clamp: palette[c * pal_w + index] is read only for 0 <= index < nb_colors <= pal_w
// and c < num_c <= pal_h, pred only where it was given.
#pragma once
#include <cstdint>

#include "../../include/jxlatte_amd.h"

namespace jxl {

// nullptr: the call is good; else what is wrong with it. out = the num_c output planes.
inline const char* palette_check(const jxl_palette_desc* d, const int32_t* index, int32_t height, int32_t width, int32_t* const* out) {
    if (!d || !index || !out) return "palette: null argument";
    if (height < 1 || width < 1) return "palette: height or width below 1";
    if ((int64_t)height * width > INT32_MAX) return "palette: more than INT32_MAX samples";
    if (d->num_c < 1) return "palette: num_c below 1";
    if (d->nb_colors < 0 || d->nb_deltas < 0) return "palette: negative nb_colors or nb_deltas";
    // ArrayIndexOutOfBoundsException at c0.buffer[c][index] (:345)
    if (d->pal_w < d->nb_colors || d->pal_h < d->num_c) return "palette: the palette channel is smaller than num_c x nb_colors";
    if (!d->palette && d->nb_colors > 0) return "palette: null palette";
    if (d->d_pred < 0 || d->d_pred > 13) return "palette: d_pred outside 0..13";
    if (d->d_pred == 6 && d->nb_deltas > 0 && !d->pred) return "palette: d_pred 6 without the weighted predictor's plane";
    if (d->bit_depth < 1 || d->bit_depth > 32) return "palette: bit_depth outside 1..32";
    for (int32_t c = 0; c < d->num_c; c++)
        if (!out[c]) return "palette: null output plane";
    return nullptr;
}

}  // namespace jxl
