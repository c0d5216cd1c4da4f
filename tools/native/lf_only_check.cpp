// LF-only decoding of the front-end (jxf_set_lf_only) as a host program of its own, for AddressSanitizer + UBSan
// (tests/test_lf_preview_cpu.py builds it from the front-end's sources with -fsanitize=address,undefined and runs it as a process).
//
//   lf_only_check FILE...             each file: decoded LF-only and in full; the LF integers, extra_precision and cell sizes must
//                                     agree, the LF-only views must have n_blocks 0 and null block maps, jxf_get_coeffs* must refuse
//   lf_only_check --prefixes FILE     every prefix length 0..size of FILE, LF-only: rejected or decoded, every integer read
//
// Prints one line per input and "<n> failure(s)"; the exit status is the number of failures (0: clean).
#include <cstdio>
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

struct Lf {
    int status = 0;  // jxf_next_frame's (or -100: jxf_open refused)
    int encoding = -1;
    std::vector<int32_t> ints;   // every LF integer of every LF group, in order
    std::vector<int32_t> shape;  // per LF group: cells_h, cells_w, extra_precision, has_lf_quant, n_blocks
    bool null_maps = true;       // every block map pointer of every view is null
    int coeffs_status = 0, sparse_status = 0;
};

// one decode of the first frame; every integer the LF views hand out is read (the sanitizer sees each load)
Lf decode(const uint8_t* data, size_t size, bool lf_only) {
    Lf r;
    char err[256];
    jxf_dec* d = jxf_open(data, size, err, sizeof err);
    if (!d) {
        r.status = -100;
        return r;
    }
    if (jxf_set_lf_only(d, lf_only ? 1 : 0) != JXF_OK) r.status = -101;
    if (r.status == 0) r.status = jxf_next_frame(d, nullptr);
    jxf_frame_info fi;
    if (r.status == JXF_OK && jxf_get_frame_info(d, &fi) == JXF_OK) {
        r.encoding = fi.encoding;
        for (int g = 0; g < fi.num_lf_groups; g++) {
            jxf_lfgroup_view v;
            if (jxf_get_lfgroup(d, g, &v) != JXF_OK) {
                r.status = -102;
                break;
            }
            r.shape.insert(r.shape.end(), {v.cells_h, v.cells_w, v.extra_precision, v.has_lf_quant, v.n_blocks});
            if (v.dct_select || v.hf_mul || v.sharpness || v.x_from_y || v.b_from_y || v.block_yx) r.null_maps = false;
            if (v.has_lf_quant)
                for (int c = 0; c < 3; c++)
                    for (int64_t i = 0; i < (int64_t)v.lf_h[c] * v.lf_w[c]; i++) r.ints.push_back(v.lf_quant[c][i]);
        }
        jxf_coeff_view cv;
        jxf_sparse_view sv;
        r.coeffs_status = jxf_get_coeffs(d, 0, 0, &cv);
        r.sparse_status = jxf_get_coeffs_sparse(d, 0, 0, &sv);
    }
    jxf_close(d);
    return r;
}

void check_file(const char* path) {
    const std::vector<uint8_t> data = slurp(path);
    if (data.empty()) return fail(std::string(path) + ": unreadable");
    const Lf a = decode(data.data(), data.size(), true), b = decode(data.data(), data.size(), false);
    if (a.status != JXF_OK || b.status != JXF_OK) return fail(std::string(path) + ": not decoded");
    if (a.encoding != 0) {  // a Modular frame ignores the switch: both decodes are the same decode
        if (a.coeffs_status == JXF_ERR_STATE) fail(std::string(path) + ": a Modular frame took the switch");
        printf("ok   %s (modular: switch ignored)\n", path);
        return;
    }
    if (a.ints != b.ints) fail(std::string(path) + ": LF integers differ from the full decode's");
    if (a.shape.size() != b.shape.size()) return fail(std::string(path) + ": LF group count");
    for (size_t i = 0; i < a.shape.size(); i += 5) {
        if (memcmp(&a.shape[i], &b.shape[i], 4 * sizeof(int32_t)) != 0) fail(std::string(path) + ": cell sizes / extra_precision differ");
        if (a.shape[i + 4] != 0) fail(std::string(path) + ": n_blocks is not 0");
        if (b.shape[i + 4] <= 0) fail(std::string(path) + ": the full decode has no blocks");
    }
    if (!a.null_maps) fail(std::string(path) + ": a block map is not null");
    if (a.coeffs_status != JXF_ERR_STATE || a.sparse_status != JXF_ERR_STATE) fail(std::string(path) + ": jxf_get_coeffs* did not refuse");
    if (b.coeffs_status != JXF_OK || b.sparse_status != JXF_OK) fail(std::string(path) + ": the full decode has no coefficients");
    printf("ok   %s (%zu LF integers)\n", path, a.ints.size());
}

void check_prefixes(const char* path) {
    const std::vector<uint8_t> data = slurp(path);
    if (data.empty()) return fail(std::string(path) + ": unreadable");
    const Lf whole = decode(data.data(), data.size(), true);
    if (whole.status != JXF_OK) return fail(std::string(path) + ": not decoded");
    size_t accepted = 0, first = 0;
    for (size_t n = 0; n <= data.size(); n++) {
        // a copy of exactly n bytes: a read past the prefix is a read past the allocation
        const std::vector<uint8_t> cut(data.begin(), data.begin() + (long)n);
        const Lf r = decode(cut.data(), cut.size(), true);
        if (r.status != JXF_OK) continue;
        if (!accepted) first = n;
        accepted++;
        if (r.ints != whole.ints) fail(std::string(path) + ": prefix " + std::to_string(n) + " decodes other integers");
    }
    if (!accepted || first >= data.size()) fail(std::string(path) + ": no proper prefix is enough");
    printf("ok   %s: %zu of %zu prefixes decode, the shortest has %zu bytes\n", path, accepted, data.size() + 1, first);
}

}  // namespace

int main(int argc, char** argv) {
    for (int i = 1; i < argc; i++) {
        if (!strcmp(argv[i], "--prefixes") && i + 1 < argc) check_prefixes(argv[++i]);
        else check_file(argv[i]);
    }
    printf("%d failure(s)\n", g_fail);
    return g_fail;
}
