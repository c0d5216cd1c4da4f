// What jxl_canvas_patches / jxl_canvas_patches_check (canvas_patch_check.h: canvas_patches_check, over patch_compile.h) and
// jxl_canvas_cast_planes (canvas_cast_list_check) refuse, as a program of its own, for the sanitizers: no device, no library.
//   g++ -std=c++17 -fsanitize=address,undefined tools/native/canvas_patch_check.cpp -o canvas_patch_check && ./canvas_patch_check
// One line per case: "REFUSAL <name> <status>" or "ACCEPT <name> <status>", then "<n> case(s), <k> failure(s)". A case fails when
// the status is not the one expected of it, a refusal gives no reason, or first_bad is not the position expected.
// tests/test_canvas_patches_cpu.py reads the lines.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>
#include <vector>

#include "../../jxlatte_amd/csrc/canvas_patch_check.h"

using namespace jxl;

namespace {

int n_cases = 0, n_fail = 0;

void report(const char* name, jxl_status want, jxl_status st, const char* why, bool extra_ok = true) {
    n_cases++;
    const bool ok = st == want && (st == JXL_OK || (why && *why)) && extra_ok;
    if (!ok) n_fail++;
    printf("%s %s %d%s\n", want == JXL_OK ? "ACCEPT" : "REFUSAL", name, (int)st, ok ? "" : " FAIL");
}

// a frame of 3 colours + 1 alpha channel, 40 x 50 floats; slot 0: 16 x 16, slot 2: 40 x 50, both four float planes; slots 1, 3 absent.
// Three positions of 8 x 8 out of slot 0, every channel blendAdd (patch mode 2). Everything is handed over as exact-size heap
// arrays: a read past one is the sanitizer's to report.
struct PatchCase {
    std::vector<jxl_patch_pos> pos;
    std::vector<int32_t> blend, is_alpha, assoc;
    jxl_patch_desc d;
    jxl_canvas_shape frame, ref[4];
    bool has_ref[4] = {true, false, true, false};
    int alias = -1;  // the slot whose shape object IS the frame's
    int32_t resident = 0;
    bool null_desc = false, null_frame = false;
    int32_t want_bad = -1;
};

jxl_canvas_shape shape(int n, int h, int w, int type) {
    jxl_canvas_shape s;
    memset(&s, 0, sizeof s);
    s.n = n, s.h = h, s.w = w;
    for (int i = 0; i < n && i < JXL_CANVAS_MAX_PLANES; i++) s.types[i] = type;
    return s;
}

void patches(const char* name, jxl_status want, const std::function<void(PatchCase&)>& edit) {
    PatchCase c;
    c.pos = {{4, 4, 8, 8, 0, 0, 0, 0}, {20, 30, 8, 8, 0, 8, 8, 0}, {32, 42, 8, 8, 0, 2, 3, 0}};
    c.blend.assign(4 * 3, 0);
    for (int ch = 0; ch < 4; ch++) c.blend[(size_t)ch * 3] = 2;
    c.is_alpha = {1};
    c.assoc = {0};
    memset(&c.d, 0, sizeof c.d);
    c.d.n_color = 3, c.d.n_extra = 1, c.d.n_rows = 1;
    for (int k = 0; k < 4; k++) c.d.ref_h[k] = c.d.ref_w[k] = 12345;  // (ignored: the sets tell)
    c.frame = shape(4, 40, 50, JXL_PLANE_FLOAT);
    c.ref[0] = shape(4, 16, 16, JXL_PLANE_FLOAT);
    c.ref[2] = shape(4, 40, 50, JXL_PLANE_FLOAT);
    c.ref[1] = c.ref[3] = shape(4, 1, 1, JXL_PLANE_FLOAT);
    edit(c);
    c.d.n_pos = (int32_t)c.pos.size();
    c.d.pos = c.pos.empty() ? nullptr : c.pos.data();
    c.d.blend = c.blend.empty() ? nullptr : c.blend.data();
    c.d.ec_is_alpha = c.is_alpha.empty() ? nullptr : c.is_alpha.data();
    c.d.ec_alpha_associated = c.assoc.empty() ? nullptr : c.assoc.data();
    const jxl_canvas_shape* rp[4];
    for (int k = 0; k < 4; k++) rp[k] = k == c.alias ? &c.frame : c.has_ref[k] ? &c.ref[k] : nullptr;
    const char* why = nullptr;
    int32_t bad = -7;
    PatchStage ps;
    const jxl_status st = canvas_patches_check(c.null_desc ? nullptr : &c.d, c.null_frame ? nullptr : &c.frame, c.resident, rp, c.alias >= 0,
                                               &ps, &why, &bad);
    bool extra = bad == c.want_bad;
    if (st == JXL_OK) {  // every list entry names a position whose rectangle is not empty
        for (int32_t i : ps.bins.list) extra = extra && i >= 0 && (size_t)i < ps.rec.size() && ps.rec[(size_t)i].y1 > ps.rec[(size_t)i].y0;
        extra = extra && ps.bins.start.size() == ps.bins.tile.size() + 1;
    }
    report(name, want, st, why, extra);
}

// three sets: 0: 5 x 7, planes int32, float, int32; 1: unknown; 2: 1 x 1, one int32 plane; 3: 64 x 96, sixteen int32 planes
void casts(const char* name, jxl_status want, const std::vector<jxl_canvas_cast_item>& items, int32_t n = INT32_MIN, bool null_items = false,
           const std::vector<int>& want_skipped = {}) {
    jxl_canvas_shape sets[4] = {shape(3, 5, 7, JXL_PLANE_INT32), shape(1, 1, 1, JXL_PLANE_INT32), shape(1, 1, 1, JXL_PLANE_INT32),
                                shape(16, 64, 96, JXL_PLANE_INT32)};
    sets[0].types[1] = JXL_PLANE_FLOAT;
    auto lookup = [&](int32_t id) -> const jxl_canvas_shape* { return id >= 0 && id < 4 && id != 1 ? &sets[id] : nullptr; };
    if (n == INT32_MIN) n = (int32_t)items.size();
    std::vector<float> scale((size_t)(n > 0 ? n : 0), -1.0f);  // exact size
    const char* why = nullptr;
    const jxl_status st = canvas_cast_list_check(n, null_items || items.empty() ? nullptr : items.data(), lookup, scale.empty() ? nullptr : scale.data(), &why);
    bool extra = true;
    if (st == JXL_OK)
        for (int32_t i = 0; i < n; i++) {
            bool skip = false;
            for (int s : want_skipped) skip = skip || s == i;
            extra = extra && (skip ? scale[(size_t)i] == 0.0f : scale[(size_t)i] == 1.0f / (float)pfm_depth_max(items[(size_t)i].depth));
        }
    report(name, want, st, why, extra);
}

}  // namespace

int main() {
    const jxl_status INV = JXL_ERR_INVALID_ARGUMENT, BIT = JXL_ERR_INVALID_BITSTREAM, UNS = JXL_ERR_UNSUPPORTED;
    // ---- jxl_canvas_patches: the set-level refusals ----
    patches("patches_null_desc", INV, [](PatchCase& c) { c.null_desc = true; });
    patches("patches_null_frame", INV, [](PatchCase& c) { c.null_frame = true; });
    patches("patches_frame_with_three_planes", INV, [](PatchCase& c) { c.frame.n = 3; });
    patches("patches_frame_with_five_planes", INV, [](PatchCase& c) { c.frame.n = 5; });
    patches("patches_slot_with_three_planes", INV, [](PatchCase& c) { c.ref[2].n = 3; });
    patches("patches_seventeen_planes", UNS, [](PatchCase& c) {
        c.d.n_extra = 14, c.frame.n = c.ref[0].n = c.ref[2].n = 17;
        c.is_alpha.assign(14, 0), c.assoc.assign(14, 0), c.blend.assign(17 * 3, 0);
    });
    patches("patches_frame_plane_type_2", INV, [](PatchCase& c) { c.frame.types[3] = 2; });
    patches("patches_slot_of_height_0", INV, [](PatchCase& c) { c.ref[0].h = 0; });
    patches("patches_resident_colours_of_a_grey_frame", INV, [](PatchCase& c) {
        c.resident = 1, c.d.n_color = 1, c.frame.n = c.ref[0].n = c.ref[2].n = 2, c.blend.assign(2 * 3, 0);
    });
    patches("patches_frame_is_slot_1", INV, [](PatchCase& c) { c.alias = 1; });
    patches("patches_frame_is_slot_0", INV, [](PatchCase& c) { c.alias = 0; });
    // ---- ... then jxl_patch_bins' validation, on the sets' sizes and types ----
    patches("patches_slot_4", BIT, [](PatchCase& c) { c.pos[1].ref = 4, c.want_bad = 1; });
    patches("patches_too_large_for_the_set", BIT, [](PatchCase& c) { c.pos[2].ref_y0 = 9, c.want_bad = 2; });
    patches("patches_outside_the_frame", BIT, [](PatchCase& c) { c.pos[0].y0 = 33, c.want_bad = 0; });
    patches("patches_negative_origin", BIT, [](PatchCase& c) { c.pos[1].x0 = -1, c.want_bad = 1; });
    patches("patches_illegal_mode", BIT, [](PatchCase& c) { c.blend[0] = 8, c.want_bad = 0; });
    patches("patches_blend_row_out_of_range", INV, [](PatchCase& c) { c.pos[2].blend = 1, c.want_bad = 2; });
    patches("patches_float_function_on_int_planes", INV, [](PatchCase& c) {
        c.frame = shape(4, 40, 50, JXL_PLANE_INT32), c.ref[0] = shape(4, 16, 16, JXL_PLANE_INT32), c.blend[0] = 3, c.want_bad = 0;
    });
    patches("patches_slot_plane_of_another_type", INV, [](PatchCase& c) { c.ref[0].types[1] = JXL_PLANE_INT32, c.want_bad = 0; });
    patches("patches_int_colours_in_the_set_under_resident_colours_with_int_slot", INV, [](PatchCase& c) {
        c.resident = 1, c.ref[0].types[0] = JXL_PLANE_INT32, c.want_bad = 0;
    });
    patches("patches_below_mode_off_its_pixel", UNS, [](PatchCase& c) { c.blend[0] = 5, c.want_bad = 0; });
    patches("patches_alpha_copy_outside_the_slot", INV, [](PatchCase& c) { c.blend[9] = 4, c.want_bad = 1; });
    // ---- accepted ----
    patches("patches_three_positions", JXL_OK, [](PatchCase&) {});
    patches("patches_no_position", JXL_OK, [](PatchCase& c) { c.pos.clear(); });
    patches("patches_absent_slot_is_skipped", JXL_OK, [](PatchCase& c) { c.pos[1] = jxl_patch_pos{-5, 99, 1000, 1000, 3, 7, 7, 0}; });
    patches("patches_two_slots_one_shape", JXL_OK, [](PatchCase& c) { c.has_ref[1] = true, c.ref[1] = c.ref[0], c.pos[1].ref = 1; });
    patches("patches_int_colours_in_the_set_under_resident_colours", JXL_OK, [](PatchCase& c) {
        c.resident = 1;
        for (int i = 0; i < 3; i++) c.frame.types[i] = JXL_PLANE_INT32;
    });
    patches("patches_below_mode_on_its_pixel", JXL_OK, [](PatchCase& c) {
        c.blend[0] = 5;
        for (auto& p : c.pos) p.ref = 2, p.ref_y0 = p.y0, p.ref_x0 = p.x0;
    });
    patches("patches_sixteen_planes", JXL_OK, [](PatchCase& c) {
        c.d.n_extra = 13, c.frame.n = c.ref[0].n = c.ref[2].n = 16;
        c.is_alpha.assign(13, 0), c.assoc.assign(13, 0), c.blend.assign(16 * 3, 0);
        for (int ch = 0; ch < 16; ch++) c.blend[(size_t)ch * 3] = 2;
    });
    // ---- jxl_canvas_cast_planes ----
    casts("cast_negative_count", INV, {}, -1);
    casts("cast_null_items", INV, {{0, 0, 8}}, 1, true);
    std::vector<jxl_canvas_cast_item> many;
    for (int i = 0; i < 81; i++) many.push_back({3, i % 16, 8});
    casts("cast_81_items", INV, many);
    casts("cast_unknown_set", INV, {{0, 0, 8}, {1, 0, 8}});
    casts("cast_negative_set", INV, {{-1, 0, 8}});
    casts("cast_plane_past_the_set", INV, {{0, 3, 8}});
    casts("cast_negative_plane", INV, {{2, -1, 8}});
    casts("cast_plane_named_twice", INV, {{0, 0, 8}, {3, 5, 8}, {0, 0, 16}});
    casts("cast_float_plane_named_twice", INV, {{0, 1, 8}, {0, 1, 8}});
    casts("cast_depth_0", INV, {{0, 0, 0}});
    casts("cast_depth_32", INV, {{3, 15, 32}});
    casts("cast_depth_64_after_good_items", INV, {{0, 0, 8}, {2, 0, 31 + 32 + 1}});  // (Java counts a shift modulo 32: depth 64 is depth 0)
    casts("cast_nothing", JXL_OK, {});
    casts("cast_depths_1_to_31", JXL_OK, {{0, 0, 1}, {0, 2, 8}, {2, 0, 12}, {3, 0, 16}, {3, 1, 24}, {3, 2, 31}});
    casts("cast_float_plane_is_skipped_whatever_its_depth", JXL_OK, {{0, 1, 0}, {0, 0, 8}}, INT32_MIN, false, {0});
    many.pop_back();
    for (int i = 0; i < 80; i++) many[(size_t)i] = {i < 16 ? 3 : 0, i < 16 ? i : 0, 8};
    many.resize(19);
    many[16] = {0, 0, 8}, many[17] = {0, 2, 8}, many[18] = {2, 0, 8};
    casts("cast_every_int_plane_of_three_sets", JXL_OK, many);
    printf("%d case(s), %d failure(s)\n", n_cases, n_fail);
    return n_fail ? 1 : 0;
}
