// modplanes_check.h (what jxl_canvas_from_modular refuses) as a program of its own, for the sanitizers: no device, no library.
//   g++ -std=c++17 -fsanitize=address,undefined tools/native/modplanes_check.cpp -o modplanes_check && ./modplanes_check
// One line per case: "REFUSAL <name> <status>" or "ACCEPT <name> <status>", then "<n> case(s), <k> failure(s)". A case fails when
// the status is not the one expected of it, or a refusal gives no reason. tests/test_modplanes_cpu.py reads the lines.
#include <cstdio>
#include <cstring>
#include <functional>
#include <vector>

#include "../../jxlatte_amd/csrc/modplanes_check.h"

using namespace jxl;

namespace {

int n_cases = 0, n_fail = 0;

// result list of every case: 0, 1, 2: 40 x 140; 3: 9 x 131; 4: 40 x 139; 5: 1 x 1; 6: 33 x 130
const std::vector<ModPlaneShape> kOut = {{40, 140}, {40, 140}, {40, 140}, {9, 131}, {40, 139}, {1, 1}, {33, 130}};

jxl_modular_planes_desc base(int h, int w, int n) {
    jxl_modular_planes_desc d;
    memset(&d, 0, sizeof d);
    d.height = h, d.width = w, d.n_planes = n;
    for (int i = 0; i < JXL_CANVAS_MAX_PLANES; i++) d.plane[i] = jxl_modular_plane{i % 3, -1, JXL_PLANE_INT32, 1.0f};
    return d;
}

void run(const char* name, jxl_status want, const std::function<void(jxl_modular_planes_desc&)>& edit, bool ran = true,
         bool null_desc = false, int32_t n_out = -1) {
    jxl_modular_planes_desc d = base(33, 130, 3);
    edit(d);
    // the list is handed over as an exact-size heap array: a read past it is the sanitizer's to report
    const int32_t n = n_out < 0 ? (int32_t)kOut.size() : n_out;
    std::vector<ModPlaneShape> out(kOut.begin(), kOut.begin() + n);
    const char* why = nullptr;
    const jxl_status st = modplanes_check(null_desc ? nullptr : &d, n ? out.data() : nullptr, n, ran, &why);
    n_cases++;
    const bool ok = st == want && (st == JXL_OK || (why && *why));
    if (!ok) n_fail++;
    printf("%s %s %d%s\n", want == JXL_OK ? "ACCEPT" : "REFUSAL", name, (int)st, ok ? "" : " FAIL");
}

}  // namespace

int main() {
    const jxl_status INV = JXL_ERR_INVALID_ARGUMENT;
    auto none = [](jxl_modular_planes_desc&) {};
    // ---- refusals ----
    run("null_desc", INV, none, true, true);
    run("no_plan_has_run", JXL_ERR_STATE, none, false);
    run("no_plan_has_run_bad_desc", JXL_ERR_STATE, [](auto& d) { d.n_planes = 0; }, false);  // the state is looked at first
    run("n_planes_0", INV, [](auto& d) { d.n_planes = 0; });
    run("n_planes_negative", INV, [](auto& d) { d.n_planes = -1; });
    run("n_planes_17", JXL_ERR_UNSUPPORTED, [](auto& d) { d.n_planes = 17; });
    run("n_planes_int_max", JXL_ERR_UNSUPPORTED, [](auto& d) { d.n_planes = INT32_MAX; });
    run("height_0", INV, [](auto& d) { d.height = 0; });
    run("width_0", INV, [](auto& d) { d.width = 0; });
    run("height_negative", INV, [](auto& d) { d.height = -5; });
    run("width_negative", INV, [](auto& d) { d.width = INT32_MIN; });
    run("channel_negative", INV, [](auto& d) { d.plane[1].channel = -1; });
    run("channel_past_the_list", INV, [](auto& d) { d.plane[2].channel = 7; });
    run("channel_int_max", INV, [](auto& d) { d.plane[0].channel = INT32_MAX; });
    run("empty_result_list", INV, none, true, false, 0);
    run("channel_lower_than_bounds", INV, [](auto& d) { d.plane[0].channel = 3; });                   // 9 rows < 33
    run("channel_narrower_than_bounds", INV, [](auto& d) { d.height = 40, d.width = 140, d.plane[0].channel = 4; });  // 139 < 140
    run("last_plane_too_small", INV, [](auto& d) { d.n_planes = 16, d.plane[15].channel = 5; });
    run("add_on_int32_plane", INV, [](auto& d) { d.plane[0].add_channel = 1; });
    run("add_channel_negative", INV, [](auto& d) { d.plane[0].type = JXL_PLANE_FLOAT, d.plane[0].add_channel = -2; });
    run("add_channel_past_the_list", INV, [](auto& d) { d.plane[0].type = JXL_PLANE_FLOAT, d.plane[0].add_channel = 7; });
    run("add_channel_other_width", INV, [](auto& d) { d.plane[0].type = JXL_PLANE_FLOAT, d.plane[0].add_channel = 4; });
    run("add_channel_other_height", INV, [](auto& d) { d.height = 9, d.plane[0].type = JXL_PLANE_FLOAT, d.plane[0].add_channel = 3; });
    run("type_2", INV, [](auto& d) { d.plane[1].type = 2; });
    run("type_negative", INV, [](auto& d) { d.plane[2].type = -1; });
    // ---- accepted edge cases ----
    run("three_int32_planes", JXL_OK, none);
    run("one_plane", JXL_OK, [](auto& d) { d.n_planes = 1; });
    run("sixteen_planes", JXL_OK, [](auto& d) { d.n_planes = 16; });
    run("bounds_1x1_of_a_1x1_channel", JXL_OK, [](auto& d) { d.height = d.width = 1, d.n_planes = 1, d.plane[0].channel = 5; });
    run("bounds_equal_to_the_channel", JXL_OK, [](auto& d) { d.height = 40, d.width = 140; });
    run("channel_larger_than_bounds", JXL_OK, [](auto& d) { d.height = 5, d.width = 7, d.plane[0].channel = 3; });
    run("last_channel_of_the_list", JXL_OK, [](auto& d) { d.plane[0].channel = 6; });
    run("one_channel_in_every_plane", JXL_OK, [](auto& d) { for (int i = 0; i < 3; i++) d.plane[i].channel = 0; });
    run("float_plane_without_add", JXL_OK, [](auto& d) { d.plane[0].type = JXL_PLANE_FLOAT; });
    run("float_plane_adds_itself", JXL_OK, [](auto& d) { d.plane[0].type = JXL_PLANE_FLOAT, d.plane[0].add_channel = 0; });
    run("xyb_mapping", JXL_OK, [](auto& d) {
        d.plane[0] = jxl_modular_plane{1, -1, JXL_PLANE_FLOAT, 0.25f};
        d.plane[1] = jxl_modular_plane{0, -1, JXL_PLANE_FLOAT, 0.5f};
        d.plane[2] = jxl_modular_plane{2, 0, JXL_PLANE_FLOAT, 0.125f};
    });
    run("planes_past_n_planes_are_not_looked_at", JXL_OK, [](auto& d) { d.plane[3] = jxl_modular_plane{99, 99, 99, 0.0f}; });
    printf("%d case(s), %d failure(s)\n", n_cases, n_fail);
    return n_fail ? 1 : 0;
}
