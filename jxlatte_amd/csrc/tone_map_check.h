// The pure part of jxl_ctx_set_tone_map (host.hip): the refusals of one jxl_tone_map and the block the kernels take, its derived
// constants computed in double and rounded once to float (tone_map_ops.h). Plain C++: no device call, no context;
// tools/native/tone_map_check.cpp runs it as a program of its own under the sanitizers.
#ifndef JXL_TONE_MAP_CHECK_H
#define JXL_TONE_MAP_CHECK_H
#include <cmath>
#include <initializer_list>
#include <stdint.h>

#include "../../include/jxlatte_amd.h"
#include "tone_map_ops.h"

namespace jxl {

// nullptr, or why the block is refused (JXL_ERR_INVALID_ARGUMENT)
inline const char* tone_map_check(const jxl_tone_map* tm) {
    if (!tm) return "tone map: null argument";
    for (float nits : {tm->unit_nits, tm->source_nits, tm->target_nits})
        if (!std::isfinite(nits) || !(nits > 0.0f)) return "tone map: the nits are finite and positive";
    if (tm->source_nits > 10000.0f) return "tone map: source_nits is at most 10000";
    double sum = 0.0;
    for (float w : tm->lum) {
        if (!std::isfinite(w)) return "tone map: a luminance weight is not finite";
        sum += (double)w;
    }
    if (!(sum > 0.0) || sum > 2.0) return "tone map: the luminance weights sum to a value in (0, 2]";
    if (tm->gamut != 0 && tm->gamut != 1) return "tone map: gamut is 0 or 1";
    return nullptr;
}

// the kernels' block of a block tone_map_check has passed
inline void tone_map_fill(const jxl_tone_map* tm, ToneMapArgs* a) {
    for (int i = 0; i < 3; i++) a->lum[i] = tm->lum[i];
    a->unit_nits = tm->unit_nits, a->source_nits = tm->source_nits, a->target_nits = tm->target_nits;
    a->gamut = tm->gamut;
    const double e_src = tm_pq_inv((double)tm->source_nits);
    const double max_lum = tm_pq_inv((double)tm->target_nits) / e_src;
    a->e_src = (float)e_src;
    a->max_lum = (float)max_lum;
    a->ks = (float)(1.5 * max_lum - 0.5);
    a->norm = (float)((double)tm->unit_nits / (double)tm->target_nits);
}

}  // namespace jxl
#endif  // JXL_TONE_MAP_CHECK_H
