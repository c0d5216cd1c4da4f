// jxl_pfm_params: what both PFM entries refuse, and the cast's scale per plane. Plain C++ (no device code, no context), so the
// checks can be compiled and run on their own.
#pragma once
#include <cstdint>

#include "../../include/jxlatte_amd.h"

namespace jxl {

// ImageBuffer.castToFloat(depth) -> castToFloat0(~(~0 << depth)): Java int arithmetic, where a shift count counts modulo 32
// (depth 32 gives 0, like depth 0)
inline int32_t pfm_depth_max(int32_t depth) { return (int32_t)~(~0u << ((uint32_t)depth & 31u)); }

// nullptr: the parameters are good and scale[c] = 1.0f / max for the int32 planes (0 for the others); else what is wrong
inline const char* pfm_check(const jxl_pfm_params* p, float scale[3]) {
    if (!p) return "pfm samples: null argument";
    if (p->height < 1 || p->width < 1) return "pfm samples: bad size";
    if (p->n_planes != 1 && p->n_planes != 3) return "pfm samples: 1 (grey) or 3 planes";
    for (int c = 0; c < 3; c++) {
        scale[c] = 0.0f;
        if (c >= p->n_planes || !p->is_int[c]) continue;
        const int32_t max = pfm_depth_max(p->tagged_depth[c]);
        if (max < 1) return "invalid Max Value";  // ImageBuffer.java:115-116
        scale[c] = 1.0f / (float)max;             // ImageBuffer.java:119
    }
    return nullptr;
}

}  // namespace jxl
