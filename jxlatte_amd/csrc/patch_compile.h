// Host side of the patch stage: JXLCodestreamDecoder.computePatches' checks (JXLCodestreamDecoder.java:212-254), the choice of the
// blend function blendBuffers makes per (position, channel) (:466-512), and the binning of the positions into the tiles of
// k_patches. Plain C++ (no device code, no device call, no context): jxl_patch_bins works without a GPU, and the checks can be
// compiled and run on their own (canvas_patch_check.h). No casts happen here: the planes come with the types blendBuffers' side
// effects (:433-465) would have given them (jxlatte_amd/decoder.py: patch_type_plan).
#pragma once
#include <cstdint>
#include <limits>
#include <new>
#include <vector>

#include "../../include/jxlatte_amd.h"
#include "blend_ops.h"

namespace jxl {

// The binned form of a table of records, as offsets (in int32 words) into one buffer the kernel reads: the non-empty tiles
// (index ty * tiles_x + tx) in raster order, per non-empty tile its CSR range, and the record indices of every tile in TABLE ORDER
// (the spline arcs of k_splines, the positions of k_patches)
struct SplineBins {
    int tiles_x = 0, tiles_y = 0;
    std::vector<int32_t> tile;   // [n_tiles]
    std::vector<int32_t> start;  // [n_tiles + 1]
    std::vector<int32_t> list;   // [start[n_tiles]]
};

constexpr int kPatchTileW = 32, kPatchTileH = 8;  // footprint of one workgroup of k_patches, as k_splines'
// one position as the kernel reads it (wave-uniform, through scalar loads): the rectangle [y0, y1) x [x0, x1) in the frame, the
// shift (dy, dx) from a frame pixel to its sample in the slot's planes, and its PatchOp row (one op per channel)
struct PatchRec { int32_t y0, x0, y1, x1, dy, dx, slot, ops; };
static_assert(sizeof(PatchRec) == 32, "patch record");
enum PatchOpKind { POP_NONE, POP_ADD_I, POP_ADD_F, POP_MULT, POP_BLEND, POP_MULADD, POP_COPY_REF };
constexpr int kPatchIsAlpha = 1, kPatchClamp = 2, kPatchPremult = 4, kPatchBelow = 8;
struct PatchOp { int32_t op, alpha, flags, reserved; };  // alpha: the channel number (n_color + alphaChannel) of the alpha planes
static_assert(sizeof(PatchOp) == 16, "patch op");
struct PatchStage {
    int n_chan = 0;
    std::vector<PatchRec> rec;     // [n_pos], stage order; a skipped position has an empty rectangle and is in no list
    std::vector<PatchOp> ops;      // rows of n_chan, one row per (blend row, slot) in use
    std::vector<uint8_t> written;  // [n_chan]: some position stores into the channel
    SplineBins bins;               // list entries index rec
};

namespace patch_detail {

struct RowInfo {
    int32_t ops = -1;        // first PatchOp of the row, or -1: not compiled yet
    bool copy_ref = false;   // some channel copies the slot's plane at FRAME coordinates (blendMulAdd on the alpha channel, :388-391)
    bool below = false;      // some channel runs with old and new swapped (:489-492)
};

// the ops of one (blend row, slot): blendBuffers' inner switch per channel, checked as jxl_stage_blend checks one call
inline jxl_status compile_row(const jxl_patch_desc* d, int row, int slot, const int32_t* frame_type, const int32_t* ref_type,
                              PatchStage* out, RowInfo* info, const char** why) {
    const int n_chan = out->n_chan;
    const bool has_extra = d->n_extra > 0;
    info->ops = (int32_t)out->ops.size();
    out->ops.resize(out->ops.size() + (size_t)n_chan, PatchOp{POP_NONE, 0, 0, 0});
    for (int ch = 0; ch < n_chan; ch++) {
        const int32_t* bi = d->blend + ((size_t)row * (size_t)n_chan + (size_t)ch) * 3;
        const int32_t mode = bi[0], alpha = bi[1], clamp = bi[2];
        if (mode == 0) continue;  // :241-242
        if (mode < 0 || mode > 7) return *why = "Illegal blend mode", JXL_ERR_INVALID_BITSTREAM;  // :510-511
        if (has_extra && (alpha < 0 || alpha >= d->n_extra)) return *why = "patches: alpha channel out of range", JXL_ERR_INVALID_ARGUMENT;
        // raw mode 1 becomes BLEND_REPLACE (:484), for which the switch of :493-512 has no case: its default throws
        if (mode == 1) return *why = "Illegal blend mode", JXL_ERR_INVALID_BITSTREAM;
        const bool is_alpha = ch >= d->n_color && d->ec_is_alpha[ch - d->n_color] != 0;  // :426
        const bool premult = has_extra && d->ec_alpha_associated[alpha] != 0;           // :431
        int pmode = mode - 1;  // :471-485
        bool below = false;
        if (mode == 5) pmode = JXL_BLEND_BLEND, below = true;
        else if (mode == 6) pmode = JXL_BLEND_MULADD;
        else if (mode == 7) pmode = JXL_BLEND_MULADD, below = true;
        const int ft = frame_type[ch];
        const unsigned flags = (is_alpha ? JXL_BLEND_FLAG_IS_ALPHA : 0u) | (has_extra ? JXL_BLEND_FLAG_HAS_EXTRA : 0u);
        const int op = blend_op(pmode, flags, ft);
        if (op == -1) return *why = "Illegal blend mode", JXL_ERR_INVALID_BITSTREAM;
        if (op == -2) return *why = "blend: this mode works on float samples", JXL_ERR_INVALID_ARGUMENT;
        // the canvas IS the frame plane and patchStart == frameOffset: copying the frame plane onto itself stores nothing new.
        // (the alpha case of MULADD copies `ref`, which is the frame plane when below; no patch mode reaches OP_COPY_FRAME)
        if (op == OP_COPY_FRAME || (op == OP_COPY_REF && below)) continue;
        bool nf, nr, nfa, nra;
        blend_needs(op, &nf, &nr, &nfa, &nra, is_alpha);
        const int rt = ref_type[slot * n_chan + ch];
        if (rt != -1 && rt != ft) return *why = "patches: a reference plane and its frame plane differ in type", JXL_ERR_INVALID_ARGUMENT;
        const int a_ch = d->n_color + alpha;
        if (nfa && frame_type[a_ch] != 0) return *why = "blend: a plane this mode reads is NULL", JXL_ERR_INVALID_ARGUMENT;  // (int alpha: not handed over)
        if (nra && ref_type[slot * n_chan + a_ch] == 1) return *why = "blend: a plane this mode reads is NULL", JXL_ERR_INVALID_ARGUMENT;
        PatchOp& o = out->ops[(size_t)info->ops + (size_t)ch];
        o.op = op == OP_ADD_I ? POP_ADD_I : op == OP_ADD_F ? POP_ADD_F : op == OP_MULT ? POP_MULT : op == OP_BLEND ? POP_BLEND
             : op == OP_MULADD ? POP_MULADD : POP_COPY_REF;
        o.alpha = has_extra ? a_ch : 0;
        o.flags = (is_alpha ? kPatchIsAlpha : 0) | (clamp ? kPatchClamp : 0) | (premult ? kPatchPremult : 0) | (below ? kPatchBelow : 0);
        if (op == OP_COPY_REF) info->copy_ref = true;
        if (below) info->below = true;
        out->written[(size_t)ch] = 1;
    }
    return JXL_OK;
}

// two passes over the records: count per tile, prefix sum, fill -- positions visited in stage order, so every list is in stage order
inline bool patch_bin(const std::vector<PatchRec>& rec, int32_t height, int32_t width, SplineBins* out) {
    try {
        const int tx_n = (width + kPatchTileW - 1) / kPatchTileW, ty_n = (height + kPatchTileH - 1) / kPatchTileH;
        out->tiles_x = tx_n;
        out->tiles_y = ty_n;
        const size_t n_all = (size_t)tx_n * ty_n;
        std::vector<int64_t> count(n_all + 1, 0);
        for (const PatchRec& r : rec) {
            if (r.y1 <= r.y0 || r.x1 <= r.x0) continue;
            for (int ty = r.y0 / kPatchTileH; ty <= (r.y1 - 1) / kPatchTileH; ty++)
                for (int tx = r.x0 / kPatchTileW; tx <= (r.x1 - 1) / kPatchTileW; tx++) count[(size_t)ty * tx_n + tx + 1]++;
        }
        for (size_t i = 0; i < n_all; i++) count[i + 1] += count[i];
        if (count[n_all] > std::numeric_limits<int32_t>::max()) return false;
        out->list.assign((size_t)count[n_all], 0);
        out->tile.clear();
        out->start.clear();
        for (size_t t = 0; t < n_all; t++)
            if (count[t + 1] > count[t]) {
                out->tile.push_back((int32_t)t);
                out->start.push_back((int32_t)count[t]);
            }
        out->start.push_back((int32_t)count[n_all]);
        for (size_t i = 0; i < rec.size(); i++) {
            const PatchRec& r = rec[i];
            if (r.y1 <= r.y0 || r.x1 <= r.x0) continue;
            for (int ty = r.y0 / kPatchTileH; ty <= (r.y1 - 1) / kPatchTileH; ty++)
                for (int tx = r.x0 / kPatchTileW; tx <= (r.x1 - 1) / kPatchTileW; tx++) out->list[(size_t)count[(size_t)ty * tx_n + tx]++] = (int32_t)i;
        }
    } catch (const std::bad_alloc&) {
        return false;
    }
    return true;
}

}  // namespace patch_detail

// JXL_OK, or the status of jxl_patch_bins with the reason in *why and the offending position in *first_bad (or -1)
inline jxl_status patch_compile(const jxl_patch_desc* d, int32_t height, int32_t width, const int32_t* frame_type, const int32_t* ref_type,
                                PatchStage* out, const char** why, int32_t* first_bad) {
    using namespace patch_detail;
    const char* dummy;
    int32_t dummy_bad;
    if (!why) why = &dummy;
    if (!first_bad) first_bad = &dummy_bad;
    *first_bad = -1;
    if (!d || d->n_pos < 0 || d->n_rows < 0 || d->n_extra < 0 || (d->n_color != 1 && d->n_color != 3) || height < 1 || width < 1 ||
        !frame_type || !ref_type || (d->n_pos > 0 && (!d->pos || !d->blend)) || (d->n_extra > 0 && (!d->ec_is_alpha || !d->ec_alpha_associated)))
        return *why = "patches: bad arguments", JXL_ERR_INVALID_ARGUMENT;
    const int n_chan = d->n_color + d->n_extra;
    for (int ch = 0; ch < n_chan; ch++)
        if (frame_type[ch] != 0 && frame_type[ch] != 1) return *why = "patches: frame plane type", JXL_ERR_INVALID_ARGUMENT;
    for (int k = 0; k < 4; k++) {
        if (d->ref_h[k] < 0 || d->ref_w[k] < 0 || (d->ref_h[k] == 0) != (d->ref_w[k] == 0)) return *why = "patches: reference size", JXL_ERR_INVALID_ARGUMENT;
        for (int ch = 0; ch < n_chan; ch++)
            if (ref_type[k * n_chan + ch] < -1 || ref_type[k * n_chan + ch] > 1) return *why = "patches: reference plane type", JXL_ERR_INVALID_ARGUMENT;
    }
    try {
        out->n_chan = n_chan;
        out->rec.assign((size_t)d->n_pos, PatchRec{0, 0, 0, 0, 0, 0, 0, 0});
        out->ops.clear();
        out->written.assign((size_t)n_chan, 0);
        std::vector<RowInfo> rows((size_t)d->n_rows * 4);
        for (int32_t i = 0; i < d->n_pos; i++) {
            const jxl_patch_pos& p = d->pos[i];
            *first_bad = i;
            if (p.ref > 3) return *why = "Patch out of range", JXL_ERR_INVALID_BITSTREAM;  // :220-221
            if (p.ref < 0 || p.h < 0 || p.w < 0 || p.ref_y0 < 0 || p.ref_x0 < 0 || p.blend < 0 || p.blend >= d->n_rows)
                return *why = "patches: bad position", JXL_ERR_INVALID_ARGUMENT;
            if (d->ref_h[p.ref] == 0) continue;  // :225-226
            if ((int64_t)p.ref_y0 + p.h > d->ref_h[p.ref] || (int64_t)p.ref_x0 + p.w > d->ref_w[p.ref])
                return *why = "Patch too large", JXL_ERR_INVALID_BITSTREAM;  // :227-229
            if (p.y0 < 0 || p.x0 < 0 || (int64_t)p.h + p.y0 > height || (int64_t)p.w + p.x0 > width)
                return *why = "Patch size out of bounds", JXL_ERR_INVALID_BITSTREAM;  // :233-237
            RowInfo& ri = rows[(size_t)p.blend * 4 + (size_t)p.ref];
            if (ri.ops < 0) {
                const jxl_status st = compile_row(d, p.blend, p.ref, frame_type, ref_type, out, &ri, why);
                if (st) return st;
            }
            // blendMulAdd's alpha case reads the slot's plane at the FRAME rectangle (:390: copyToCanvas with frameOffset)
            if (ri.copy_ref && ((int64_t)p.y0 + p.h > d->ref_h[p.ref] || (int64_t)p.x0 + p.w > d->ref_w[p.ref]))
                return *why = "blend: rectangle outside a plane", JXL_ERR_INVALID_ARGUMENT;
            // a below mode hands the slot's plane over as `frame` (read at frameOffset) and the frame plane as `ref` (read at
            // refOffset): only where both rectangles are the lane's own pixel is the frame read where it is written
            if (ri.below && (d->ref_h[p.ref] != height || d->ref_w[p.ref] != width || p.ref_y0 != p.y0 || p.ref_x0 != p.x0))
                return *why = "patches: a below mode reads the frame away from the pixel it writes", JXL_ERR_UNSUPPORTED;
            out->rec[(size_t)i] = PatchRec{p.y0, p.x0, p.y0 + p.h, p.x0 + p.w, p.ref_y0 - p.y0, p.ref_x0 - p.x0, p.ref, ri.ops};
        }
        *first_bad = -1;
        if (!patch_bin(out->rec, height, width, &out->bins)) return *why = "patches: the tile lists do not fit", JXL_ERR_OOM;
    } catch (const std::bad_alloc&) {
        return *why = "patches: host allocation failed", JXL_ERR_OOM;
    }
    return JXL_OK;
}

}  // namespace jxl
