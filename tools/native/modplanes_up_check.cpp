// What jxl_canvas_from_modular_up (modplanes_check.h: modplanes_up_check) and jxl_canvas_take_planes (canvas_check.h:
// canvas_take_check) refuse, as a program of its own, for the sanitizers: no device, no library.
//   g++ -std=c++17 -fsanitize=address,undefined tools/native/modplanes_up_check.cpp -o modplanes_up_check && ./modplanes_up_check
// One line per case: "REFUSAL <name> <status>" or "ACCEPT <name> <status>", then "<n> case(s), <k> failure(s)". A case fails when
// the status is not the one expected of it, or a refusal gives no reason. tests/test_device_frames_cpu.py reads the lines.
#include <cstdio>
#include <cstring>
#include <functional>
#include <vector>

#include "../../jxlatte_amd/csrc/canvas_check.h"
#include "../../jxlatte_amd/csrc/modplanes_check.h"

using namespace jxl;

namespace {

int n_cases = 0, n_fail = 0;

// result list of every case: 0, 1, 2: 40 x 140; 3: 9 x 131; 4: 40 x 139; 5: 1 x 1; 6: 33 x 130; 7: a channel of 2^29 x 2^29
const std::vector<ModPlaneShape> kOut = {{40, 140}, {40, 140}, {40, 140}, {9, 131}, {40, 139}, {1, 1}, {33, 130}, {1 << 29, 1 << 29}};

void report(const char* name, jxl_status want, jxl_status st, const char* why) {
    n_cases++;
    const bool ok = st == want && (st == JXL_OK || (why && *why));
    if (!ok) n_fail++;
    printf("%s %s %d%s\n", want == JXL_OK ? "ACCEPT" : "REFUSAL", name, (int)st, ok ? "" : " FAIL");
}

struct UpCase {
    jxl_modular_planes_desc d;
    int32_t k = 2;
    bool weights = true, ran = true, null_desc = false;
    int32_t n_out = -1;
};

// three float planes of 33 x 130, k = 2, weights there, a plan has run
void up(const char* name, jxl_status want, const std::function<void(UpCase&)>& edit) {
    UpCase c;
    memset(&c.d, 0, sizeof c.d);
    c.d.height = 33, c.d.width = 130, c.d.n_planes = 3;
    for (int i = 0; i < JXL_CANVAS_MAX_PLANES; i++) c.d.plane[i] = jxl_modular_plane{i % 3, -1, JXL_PLANE_FLOAT, 0.25f};
    edit(c);
    // the list is handed over as an exact-size heap array: a read past it is the sanitizer's to report
    const int32_t n = c.n_out < 0 ? (int32_t)kOut.size() : c.n_out;
    std::vector<ModPlaneShape> out(kOut.begin(), kOut.begin() + n);
    const char* why = nullptr;
    const jxl_status st = modplanes_up_check(c.null_desc ? nullptr : &c.d, n ? out.data() : nullptr, n, c.ran, c.k, c.weights, &why);
    report(name, want, st, why);
}

// a set of four planes, 20 x 30, two int32 and two float; resident planes of 20 x 30
void take(const char* name, jxl_status want, const std::function<void(jxl_canvas_shape&, bool&, int32_t&, int32_t&)>& edit) {
    jxl_canvas_shape s;
    memset(&s, 0, sizeof s);
    s.n = 4, s.h = 20, s.w = 30;
    s.types[0] = s.types[1] = JXL_PLANE_INT32;
    bool known = true;
    int32_t ph = 20, pw = 30;
    edit(s, known, ph, pw);
    const char* why = nullptr;
    const jxl_status st = canvas_take_check(known ? &s : nullptr, ph, pw, &why);
    report(name, want, st, why);
}

}  // namespace

int main() {
    const jxl_status INV = JXL_ERR_INVALID_ARGUMENT;
    // ---- jxl_canvas_from_modular_up: what jxl_canvas_from_modular refuses ----
    up("up_null_desc", INV, [](UpCase& c) { c.null_desc = true; });
    up("up_no_plan_has_run", JXL_ERR_STATE, [](UpCase& c) { c.ran = false; });
    up("up_no_plan_has_run_bad_k", JXL_ERR_STATE, [](UpCase& c) { c.ran = false, c.k = 3; });  // the state is looked at first
    up("up_n_planes_0", INV, [](UpCase& c) { c.d.n_planes = 0; });
    up("up_n_planes_17", JXL_ERR_UNSUPPORTED, [](UpCase& c) { c.d.n_planes = 17; });
    up("up_height_0", INV, [](UpCase& c) { c.d.height = 0; });
    up("up_width_negative", INV, [](UpCase& c) { c.d.width = INT32_MIN; });
    up("up_channel_negative", INV, [](UpCase& c) { c.d.plane[1].channel = -1; });
    up("up_channel_past_the_list", INV, [](UpCase& c) { c.d.plane[2].channel = 8; });
    up("up_empty_result_list", INV, [](UpCase& c) { c.n_out = 0; });
    up("up_channel_lower_than_bounds", INV, [](UpCase& c) { c.d.plane[0].channel = 3; });
    up("up_channel_narrower_than_bounds", INV, [](UpCase& c) { c.d.height = 40, c.d.width = 140, c.d.plane[0].channel = 4; });
    up("up_add_channel_past_the_list", INV, [](UpCase& c) { c.d.plane[0].add_channel = 8; });
    up("up_add_channel_other_size", INV, [](UpCase& c) { c.d.plane[0].add_channel = 4; });
    up("up_type_2", INV, [](UpCase& c) { c.d.plane[1].type = 2; });
    // ---- ... and what the upsampling adds ----
    up("up_k_0", INV, [](UpCase& c) { c.k = 0; });
    up("up_k_1", INV, [](UpCase& c) { c.k = 1; });
    up("up_k_3", INV, [](UpCase& c) { c.k = 3; });
    up("up_k_16", INV, [](UpCase& c) { c.k = 16; });
    up("up_k_negative", INV, [](UpCase& c) { c.k = -2; });
    up("up_k_int_min", INV, [](UpCase& c) { c.k = INT32_MIN; });
    up("up_null_weights", INV, [](UpCase& c) { c.weights = false; });
    up("up_int32_plane", INV, [](UpCase& c) { c.d.plane[0].type = JXL_PLANE_INT32; });
    up("up_last_plane_int32", INV, [](UpCase& c) { c.d.n_planes = 16, c.d.plane[15].type = JXL_PLANE_INT32; });
    up("up_height_beyond_a_set", INV, [](UpCase& c) { c.d.height = 1 << 29, c.d.width = 1, c.k = 4, c.d.n_planes = 1, c.d.plane[0].channel = 7; });
    up("up_width_beyond_a_set", INV, [](UpCase& c) { c.d.height = 1, c.d.width = 1 << 28, c.k = 8, c.d.n_planes = 1, c.d.plane[0].channel = 7; });
    // ---- accepted ----
    up("up_three_float_planes_k2", JXL_OK, [](UpCase&) {});
    up("up_k4", JXL_OK, [](UpCase& c) { c.k = 4; });
    up("up_k8", JXL_OK, [](UpCase& c) { c.k = 8; });
    up("up_one_plane", JXL_OK, [](UpCase& c) { c.d.n_planes = 1; });
    up("up_sixteen_planes", JXL_OK, [](UpCase& c) { c.d.n_planes = 16; });
    up("up_bounds_1x1", JXL_OK, [](UpCase& c) { c.d.height = c.d.width = 1, c.d.n_planes = 1, c.d.plane[0].channel = 5, c.k = 8; });
    up("up_channel_larger_than_bounds", JXL_OK, [](UpCase& c) { c.d.height = 5, c.d.width = 7, c.d.plane[0].channel = 3; });
    up("up_plane_adds_a_channel", JXL_OK, [](UpCase& c) { c.d.plane[2].add_channel = 0; });
    up("up_largest_size_a_set_holds", JXL_OK, [](UpCase& c) { c.d.height = (1 << 28) - 1, c.d.width = 1, c.k = 8, c.d.n_planes = 1, c.d.plane[0].channel = 7; });
    up("up_planes_past_n_planes_are_not_looked_at", JXL_OK, [](UpCase& c) { c.d.plane[3] = jxl_modular_plane{99, 99, JXL_PLANE_INT32, 0.0f}; });
    // ---- jxl_canvas_take_planes ----
    take("take_unknown_set", INV, [](auto&, bool& known, auto&, auto&) { known = false; });
    take("take_unknown_set_without_planes", INV, [](auto&, bool& known, int32_t& ph, int32_t& pw) { known = false, ph = pw = 0; });
    take("take_one_plane", INV, [](jxl_canvas_shape& s, auto&, auto&, auto&) { s.n = 1; });
    take("take_two_planes", INV, [](jxl_canvas_shape& s, auto&, auto&, auto&) { s.n = 2; });
    take("take_no_resident_planes", JXL_ERR_STATE, [](auto&, auto&, int32_t& ph, int32_t& pw) { ph = pw = 0; });
    take("take_planes_higher", INV, [](auto&, auto&, int32_t& ph, auto&) { ph = 21; });
    take("take_planes_narrower", INV, [](auto&, auto&, auto&, int32_t& pw) { pw = 29; });
    take("take_planes_transposed", INV, [](auto&, auto&, int32_t& ph, int32_t& pw) { ph = 30, pw = 20; });
    take("take_set_of_four", JXL_OK, [](auto&, auto&, auto&, auto&) {});
    take("take_set_of_three", JXL_OK, [](jxl_canvas_shape& s, auto&, auto&, auto&) { s.n = 3; });
    take("take_set_of_sixteen_int32", JXL_OK, [](jxl_canvas_shape& s, auto&, auto&, auto&) {
        s.n = 16;
        for (int i = 0; i < 16; i++) s.types[i] = JXL_PLANE_INT32;
    });
    printf("%d case(s), %d failure(s)\n", n_cases, n_fail);
    return n_fail ? 1 : 0;
}
