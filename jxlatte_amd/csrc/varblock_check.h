// jxl_varblock_desc: what both varblock entries refuse, the cell map the kernel reads and the 27 x 3 tint factors of
// Frame.drawVarblocks (Frame.java:464-503). Plain C++ (no device code, no context), so all of it can be compiled and run on its
// own (tools/native/varblock_check.cpp).
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/jxl_transform_types.h"
#include "../../include/jxlatte_amd.h"

namespace jxl {

// one byte per 8 x 8 cell of the frame
constexpr uint8_t kVbTypeMask = 0x1f;  // bits 0-4: the transform type of the block that owns the cell
constexpr uint8_t kVbTopRow = 0x20;    // bit 5: the cell lies in its block's top cell row
constexpr uint8_t kVbLeftCol = 0x40;   // bit 6: the cell lies in its block's left cell column
constexpr uint8_t kVbNoBlock = 0xff;   // the cell belongs to no block
constexpr int kVbTypes = 27;

// nullptr: the descriptor is good and map holds cells_h * cells_w bytes; else what is wrong (map's contents are then unspecified).
// Refused: a null pointer, a cell grid below 1 x 1 or of more than INT32_MAX cells, a negative block count, a type outside
// 0..26, a block that leaves the cell grid, two blocks that claim one cell.
inline const char* varblock_cell_map(const jxl_varblock_desc* d, std::vector<uint8_t>* map) {
    if (!d || !map) return "varblocks: null argument";
    if (d->cells_h < 1 || d->cells_w < 1) return "varblocks: bad cell grid";
    if ((int64_t)d->cells_h * d->cells_w > INT32_MAX) return "varblocks: the cell grid is too large";
    if (d->n_blocks < 0 || (d->n_blocks > 0 && !d->blocks)) return "varblocks: bad block list";
    map->assign((size_t)d->cells_h * d->cells_w, kVbNoBlock);
    for (int32_t i = 0; i < d->n_blocks; i++) {
        const int32_t cy = d->blocks[3 * (size_t)i], cx = d->blocks[3 * (size_t)i + 1], type = d->blocks[3 * (size_t)i + 2];
        if (type < 0 || type >= kVbTypes) return "varblocks: a transform type above 26";
        const int32_t bh = JXL_TT[type].ph >> 3, bw = JXL_TT[type].pw >> 3;
        // (differences, not sums: cy + bh could pass INT32_MAX on a grid that tall)
        if (cy < 0 || cx < 0 || cy >= d->cells_h || cx >= d->cells_w || bh > d->cells_h - cy || bw > d->cells_w - cx)
            return "varblocks: a block leaves the cell grid";
        for (int32_t y = 0; y < bh; y++) {
            uint8_t* row = map->data() + (size_t)(cy + y) * d->cells_w + cx;
            for (int32_t x = 0; x < bw; x++) {
                if (row[x] != kVbNoBlock) return "varblocks: two blocks claim one cell";
                row[x] = (uint8_t)(type | (y == 0 ? kVbTopRow : 0) | (x == 0 ? kVbLeftCol : 0));
            }
        }
    }
    return nullptr;
}

// rFactor, gFactor, bFactor of every transform type (Frame.java:476-479), with Java's steps: float products, Math.cos on the
// float widened to double and its result cast back, 2f * (float)Math.PI / 3f evaluated left to right
inline void varblock_factors(float out[kVbTypes * 3]) {
    const float phi_bar = (float)(std::sqrt(5.0) * 0.5 - 0.5);  // MathHelper.PHI_BAR
    const float pi = (float)3.141592653589793;                   // (float)Math.PI
    for (int t = 0; t < kVbTypes; t++) {
        const float turn = std::fmod((float)t * phi_bar, 1.0f);  // float %: exact
        const float hue = turn * 2.0f * pi;
        const float g_shift = 2.0f * pi / 3.0f, b_shift = 4.0f * pi / 3.0f;
        const float hg = hue - g_shift, hb = hue - b_shift;
        out[3 * t + 0] = ((float)std::cos((double)hue) + 0.5f) / 1.5f;
        out[3 * t + 1] = ((float)std::cos((double)hg) + 1.0f) / 2.0f;
        out[3 * t + 2] = ((float)std::cos((double)hb) + 1.0f) / 2.0f;
    }
}

}  // namespace jxl
