// k_lf_image.hip's arguments (lf_image_host.hip fills them): the group table and all LF groups' integers lie in ONE device block.
#pragma once
#include "jxl_internal.h"

namespace jxl {

// one LF group, at table index gy * gcols + gx
struct LfImageGroup {
    int64_t q_off[3];  // its X, Y, B planes ([H][W] int32) in LfImageArgs::ints
    int32_t H, W;      // cells
    float sd[3];       // scaledDequant[i] / (1 << extraPrecision)
    float sd_gap[3];   // scaledDequant[i]
    float kX, kB;      // baseCorrelation + (factorLF - 128) / colorFactor
    int32_t smooth, reserved;
};
static_assert(sizeof(LfImageGroup) % 8 == 0, "the integers behind the table stay 8-byte aligned");

struct LfImageArgs {
    const LfImageGroup* groups;
    const int32_t* ints;
    float* out[3];  // H x W each
    int32_t H, W;   // the output in cells
    int32_t gcols;  // LF groups per row of the grid
    int32_t xyb;    // != 0: invert_xyb_px with xybp
    XybParams xybp;
};

void launch_lf_image(const LfImageArgs& a, hipStream_t s);

}  // namespace jxl
