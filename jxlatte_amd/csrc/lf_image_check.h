// The pure part of the LF-image entries (lf_image_host.hip: jxl_planes_from_lf, jxl_stage_lf_image): what a jxl_lf_image_desc must
// satisfy before anything is allocated or queued, and where each LF group lies in the one block that goes up. Plain C++: no device
// call, no context; tools/native/lf_image_check.cpp runs it as a program of its own under the sanitizers.
//
// The kernel finds a cell's LF group from (y >> 8, x >> 8) and indexes that group's integers with the group's own width, so the
// rules here are the kernel's bounds: every grid position has exactly one group, and that group has exactly the cells of its
// 256 x 256 tile of the output.
#ifndef JXL_LF_IMAGE_CHECK_H
#define JXL_LF_IMAGE_CHECK_H
#include <stdint.h>
#include <vector>

#include "../../include/jxlatte_amd.h"

namespace jxl {

constexpr int kLfGroupCells = 256;                 // the LF-group pitch in cells (2048 pixels)
constexpr int64_t kLfImageMaxCells = (int64_t)1 << 24;  // 2^30 pixels: above any frame the front-end accepts (2^28)

// The plan of an accepted descriptor: order[gy * gcols + gx] = the index in d->groups of the LF group at that position; its three
// planes start at q_off[3 * position + c] int32s into the block of all groups' integers, total_ints long
struct LfImagePlan {
    int grows = 0, gcols = 0;
    std::vector<int> order;
    std::vector<int64_t> q_off;
    int64_t total_ints = 0;
};

// nullptr, or why the descriptor is refused. out: the host planes of jxl_stage_lf_image, or nullptr for jxl_planes_from_lf
inline const char* lf_image_check(const jxl_lf_image_desc* d, const float* const* out, bool need_out, LfImagePlan* plan) {
    if (!d || !d->groups) return "lf image: null argument";
    if (need_out && (!out || !out[0] || !out[1] || !out[2])) return "lf image: null output plane";
    if (d->cells_h < 1 || d->cells_w < 1 || (int64_t)d->cells_h * d->cells_w > kLfImageMaxCells) return "lf image: the output size is out of range";
    if (d->color_factor == 0) return "lf image: color_factor is 0";
    const int grows = (d->cells_h + kLfGroupCells - 1) / kLfGroupCells, gcols = (d->cells_w + kLfGroupCells - 1) / kLfGroupCells;
    if (d->n_groups != grows * gcols) return "lf image: the group count is not the grid's";
    plan->grows = grows;
    plan->gcols = gcols;
    plan->order.assign((size_t)d->n_groups, -1);
    plan->q_off.assign((size_t)d->n_groups * 3, 0);
    for (int i = 0; i < d->n_groups; i++) {
        const jxl_lfquant_desc& g = d->groups[i];
        if (g.lfg_y < 0 || g.lfg_y >= grows || g.lfg_x < 0 || g.lfg_x >= gcols) return "lf image: an LF group lies outside the grid";
        if (g.cells_h < 1 || g.cells_w < 1 || g.cells_h > kLfGroupCells || g.cells_w > kLfGroupCells) return "lf image: bad LF group size";
        const int eh = d->cells_h - g.lfg_y * kLfGroupCells < kLfGroupCells ? d->cells_h - g.lfg_y * kLfGroupCells : kLfGroupCells;
        const int ew = d->cells_w - g.lfg_x * kLfGroupCells < kLfGroupCells ? d->cells_w - g.lfg_x * kLfGroupCells : kLfGroupCells;
        if (g.cells_h != eh || g.cells_w != ew) return "lf image: an LF group is not the size of its tile of the output";
        if (!g.lf_quant[0] || !g.lf_quant[1] || !g.lf_quant[2]) return "lf image: null LF plane";
        if (g.extra_precision < 0 || g.extra_precision > 3) return "lf image: extra_precision is out of range";
        int& slot = plan->order[(size_t)g.lfg_y * gcols + g.lfg_x];
        if (slot >= 0) return "lf image: two LF groups at one position";
        slot = i;
    }
    // (n_groups positions, each in range, none twice: every position has its group)
    int64_t at = 0;
    for (int p = 0; p < d->n_groups; p++) {
        const jxl_lfquant_desc& g = d->groups[plan->order[(size_t)p]];
        for (int c = 0; c < 3; c++) {
            plan->q_off[(size_t)p * 3 + c] = at;
            at += (int64_t)g.cells_h * g.cells_w;
        }
    }
    plan->total_ints = at;  // = 3 * cells_h * cells_w
    return nullptr;
}

}  // namespace jxl
#endif  // JXL_LF_IMAGE_CHECK_H
