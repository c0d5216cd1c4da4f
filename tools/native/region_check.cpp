// Region decoding of the front-end (jxf_set_region) as a host program of its own, for AddressSanitizer + UBSan
// (tests/test_region_cpu.py builds it from the front-end's sources with -fsanitize=address,undefined and runs it as a process).
//
//   region_check [--cut N] [--margin M] FILE X0 Y0 W H ...
//
// Each FILE with its box: the first frame is decoded in full and with the box set. What the plan says was read must be there and
// equal the full decode's -- every LF integer, every entry of the block maps, every coefficient and sparse entry is read, so the
// sanitizer sees each load -- and what was not read must answer JXF_ERR_STATE. --cut N: the region decode runs on a copy of the
// first N bytes only (a read past them is a read past the allocation) and must give the same. --margin M: jxf_debug_set_region_margin.
// Both hold for the files that follow. Prints one line per file,
//   ok FILE applied groups_read groups_total lf_groups_read lf_groups_total bytes_read bytes_total
// and "<n> failure(s)"; the exit status is the number of failures (0: clean).
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/jxlatte_frontend.h"

namespace {

int g_fail = 0;
void fail(const std::string& what) {
    printf("FAIL %s\n", what.c_str());
    g_fail++;
}

std::vector<uint8_t> slurp(const char* path) {
    std::vector<uint8_t> v;
    FILE* f = fopen(path, "rb");
    if (!f) return v;
    uint8_t buf[65536];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + n);
    fclose(f);
    return v;
}

struct Decoded {
    int status = 0;
    jxf_frame_info fi;
    jxf_region_plan plan;
    std::vector<int> lf_status, group_status;    // per LF group / per (pass, group): the accessor's answer
    std::vector<std::vector<int64_t>> lf, group;  // everything the views hand out, as numbers
};

Decoded decode(const uint8_t* data, size_t size, const int* box, int margin) {
    Decoded r;
    memset(&r.fi, 0, sizeof r.fi);
    memset(&r.plan, 0, sizeof r.plan);
    char err[256];
    jxf_dec* d = jxf_open(data, size, err, sizeof err);
    if (!d) {
        r.status = -100;
        return r;
    }
    if (box && jxf_set_region(d, box[0], box[1], box[2], box[3]) != JXF_OK) r.status = -101;
    if (box && margin >= 0 && jxf_debug_set_region_margin(d, margin) != JXF_OK) r.status = -101;
    if (r.status == 0) r.status = jxf_next_frame(d, nullptr);
    if (r.status == JXF_OK && jxf_get_frame_info(d, &r.fi) == JXF_OK && jxf_get_region_plan(d, &r.plan) == JXF_OK) {
        for (int g = 0; g < r.fi.num_lf_groups; g++) {
            jxf_lfgroup_view v;
            r.lf_status.push_back(jxf_get_lfgroup(d, g, &v));
            r.lf.emplace_back();
            if (r.lf_status.back() != JXF_OK) continue;
            std::vector<int64_t>& o = r.lf.back();
            o.insert(o.end(), {v.cells_h, v.cells_w, v.extra_precision, v.has_lf_quant, v.n_blocks});
            const int64_t cells = (int64_t)v.cells_h * v.cells_w, tiles = (int64_t)((v.cells_h + 7) / 8) * ((v.cells_w + 7) / 8);
            if (v.has_lf_quant)
                for (int c = 0; c < 3; c++)
                    for (int64_t i = 0; i < (int64_t)v.lf_h[c] * v.lf_w[c]; i++) o.push_back(v.lf_quant[c][i]);
            if (r.fi.encoding != 0) continue;  // (a Modular frame's LF groups have no block maps)
            for (int64_t i = 0; i < cells; i++) o.insert(o.end(), {v.dct_select[i], v.hf_mul[i], v.sharpness[i]});
            for (int64_t i = 0; i < tiles; i++) o.insert(o.end(), {v.x_from_y[i], v.b_from_y[i]});
            for (int64_t i = 0; i < 2 * (int64_t)v.n_blocks; i++) o.push_back(v.block_yx[i]);
        }
        if (r.fi.encoding == 0)
            for (int p = 0; p < r.fi.num_passes; p++)
                for (int g = 0; g < r.fi.num_groups; g++) {
                    jxf_coeff_view cv;
                    jxf_sparse_view sv;
                    const int a = jxf_get_coeffs(d, p, g, &cv), b = jxf_get_coeffs_sparse(d, p, g, &sv);
                    r.group_status.push_back(a == b ? a : -102);
                    r.group.emplace_back();
                    if (a != JXF_OK || b != JXF_OK) continue;
                    std::vector<int64_t>& o = r.group.back();
                    for (int c = 0; c < 3; c++) {
                        for (int64_t i = 0; i < (int64_t)cv.h[c] * cv.w[c]; i++) o.push_back(cv.q[c][i]);
                        for (int64_t i = 0; i < (int64_t)sv.n[c] * (sv.wide[c] ? 2 : 1); i++) o.push_back(sv.entries[c][i]);
                    }
                }
    }
    jxf_close(d);
    return r;
}

void check(const char* path, const int* box, long cut, int margin) {
    const std::vector<uint8_t> data = slurp(path);
    if (data.empty()) return fail(std::string(path) + ": unreadable");
    const Decoded full = decode(data.data(), data.size(), nullptr, -1);
    if (full.status != JXF_OK) return fail(std::string(path) + ": not decoded in full");
    if (cut > (long)data.size()) return fail(std::string(path) + ": --cut behind the end of the file");
    const std::vector<uint8_t> part(data.begin(), data.begin() + (cut >= 0 ? cut : (long)data.size()));  // an allocation of exactly that size
    const Decoded r = decode(part.data(), part.size(), box, margin);
    if (r.status != JXF_OK) return fail(std::string(path) + ": the region decode failed with status " + std::to_string(r.status));
    const jxf_region_plan& p = r.plan;
    if (full.plan.applied || full.plan.groups_read != full.fi.num_groups) fail(std::string(path) + ": the full decode reports a selection");
    if (p.groups_total != r.fi.num_groups || p.lf_groups_total != r.fi.num_lf_groups) fail(std::string(path) + ": the plan's totals");
    if (p.groups_read != p.group_w * p.group_h || p.lf_groups_read != p.lf_group_w * p.lf_group_h) fail(std::string(path) + ": the plan's counts");
    if (!p.applied && (p.groups_read != p.groups_total || p.section_bytes_read != p.section_bytes_total)) fail(std::string(path) + ": a whole decode that read less");
    if (p.section_bytes_read > p.section_bytes_total) fail(std::string(path) + ": more bytes read than the frame has");
    for (int g = 0; g < r.fi.num_lf_groups; g++) {
        const int y = g / r.fi.lf_group_cols, x = g % r.fi.lf_group_cols;
        const bool in = y >= p.lf_group_y0 && y < p.lf_group_y0 + p.lf_group_h && x >= p.lf_group_x0 && x < p.lf_group_x0 + p.lf_group_w;
        if (in ? (r.lf_status[g] != JXF_OK || r.lf[g] != full.lf[g]) : r.lf_status[g] != JXF_ERR_STATE)
            fail(std::string(path) + ": LF group " + std::to_string(g) + (in ? " differs from the full decode's" : " was not refused"));
    }
    for (size_t i = 0; i < r.group_status.size(); i++) {
        const int g = (int)(i % (size_t)r.fi.num_groups), y = g / r.fi.group_cols, x = g % r.fi.group_cols;
        const bool in = y >= p.group_y0 && y < p.group_y0 + p.group_h && x >= p.group_x0 && x < p.group_x0 + p.group_w;
        if (in ? (r.group_status[i] != JXF_OK || r.group[i] != full.group[i]) : r.group_status[i] != JXF_ERR_STATE)
            fail(std::string(path) + ": group " + std::to_string(g) + (in ? " differs from the full decode's" : " was not refused"));
    }
    printf("ok %s %d %d %d %d %d %" PRId64 " %" PRId64 "\n", path, p.applied, p.groups_read, p.groups_total, p.lf_groups_read, p.lf_groups_total,
           p.section_bytes_read, p.section_bytes_total);
}

}  // namespace

int main(int argc, char** argv) {
    long cut = -1;
    int margin = -1;
    for (int i = 1; i < argc; i++) {
        if (!strcmp(argv[i], "--cut") && i + 1 < argc) cut = atol(argv[++i]);
        else if (!strcmp(argv[i], "--margin") && i + 1 < argc) margin = atoi(argv[++i]);
        else if (i + 4 < argc) {
            const int box[4] = {atoi(argv[i + 1]), atoi(argv[i + 2]), atoi(argv[i + 3]), atoi(argv[i + 4])};
            check(argv[i], box, cut, margin);
            i += 4;
        } else {
            fail(std::string("arguments: ") + argv[i]);
        }
    }
    printf("%d failure(s)\n", g_fail);
    return g_fail;
}
