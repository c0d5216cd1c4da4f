// Stand-alone host check of jxlatte_amd/csrc/palette_ops.h and palette_check.h (no device, no context), meant for an
// AddressSanitizer + UBSan build (tests/test_palette_cpu.py):
//   * runs the validator over what jxl_stage_palette refuses, one line each ("REFUSAL <name> ok" / "FAIL ...")
//   * with a case file as argv[1] and an output file as argv[2]: undoes every case's palette with a host loop in the reference's
//     order (ModularStream.java:337-372: channel by channel, raster order) over palette_value and palette_predict, and writes the
//     num_c planes of every case, back to back, as raw int32
// Case file (raw int32, native byte order): the case count, then per case the ten words h, w, num_c, nb_colors, nb_deltas, d_pred,
// bit_depth, pal_h, pal_w, has_pred, then h * w indices, pal_h * pal_w palette entries and, if has_pred, h * w predictor values.
// Every array is copied into an allocation of exactly its size, so a read past one is the sanitizer's to find.
// Ends with "<n> case(s)" and "<n> failure(s)".
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../jxlatte_amd/csrc/palette_check.h"
#include "../../jxlatte_amd/csrc/palette_ops.h"

static int failures = 0;

static void refusal(const char* name, bool refused) {
    if (refused) {
        printf("REFUSAL %s ok\n", name);
    } else {
        printf("FAIL: %s was accepted\n", name);
        failures++;
    }
}

static void refusals() {
    int32_t index[6] = {0, 1, 2, 0, 1, 2}, palette[12] = {0}, pred[6] = {0}, o0[6], o1[6];
    int32_t* out[2] = {o0, o1};
    const jxl_palette_desc good = {2, 3, 1, 5, 8, 2, 3, palette, pred};
    if (jxl::palette_check(&good, index, 2, 3, out)) {
        printf("FAIL: a good call was refused: %s\n", jxl::palette_check(&good, index, 2, 3, out));
        failures++;
    }
    jxl_palette_desc d = good;
    refusal("null_desc", jxl::palette_check(nullptr, index, 2, 3, out));
    refusal("null_index", jxl::palette_check(&good, nullptr, 2, 3, out));
    refusal("null_out", jxl::palette_check(&good, index, 2, 3, nullptr));
    int32_t* hole[2] = {o0, nullptr};
    refusal("null_out_plane", jxl::palette_check(&good, index, 2, 3, hole));
    d.palette = nullptr;
    refusal("null_palette", jxl::palette_check(&d, index, 2, 3, out));
    d = good;
    refusal("height_0", jxl::palette_check(&good, index, 0, 3, out));
    refusal("width_0", jxl::palette_check(&good, index, 2, 0, out));
    refusal("height_negative", jxl::palette_check(&good, index, -2, 3, out));
    refusal("width_negative", jxl::palette_check(&good, index, 2, INT32_MIN, out));
    refusal("too_many_samples", jxl::palette_check(&good, index, 65536, 32768, out));  // 2^31 = INT32_MAX + 1
    refusal("too_many_samples_max", jxl::palette_check(&good, index, INT32_MAX, INT32_MAX, out));
    d.num_c = 0;
    refusal("num_c_0", jxl::palette_check(&d, index, 2, 3, out));
    d.num_c = -1;
    refusal("num_c_negative", jxl::palette_check(&d, index, 2, 3, out));
    d = good;
    d.nb_colors = -1;
    refusal("nb_colors_negative", jxl::palette_check(&d, index, 2, 3, out));
    d = good;
    d.nb_deltas = -1;
    refusal("nb_deltas_negative", jxl::palette_check(&d, index, 2, 3, out));
    d = good;
    d.pal_w = 2;
    refusal("pal_w_below_nb_colors", jxl::palette_check(&d, index, 2, 3, out));
    d = good;
    d.pal_h = 1;
    refusal("pal_h_below_num_c", jxl::palette_check(&d, index, 2, 3, out));
    d = good;
    d.d_pred = -1;
    refusal("d_pred_negative", jxl::palette_check(&d, index, 2, 3, out));
    d.d_pred = 14;
    refusal("d_pred_14", jxl::palette_check(&d, index, 2, 3, out));
    d = good;
    d.d_pred = 6;
    d.pred = nullptr;
    refusal("d_pred_6_without_pred", jxl::palette_check(&d, index, 2, 3, out));
    d.nb_deltas = 0;  // no positive delta index can name the plane: accepted (a negative index then adds 0)
    if (jxl::palette_check(&d, index, 2, 3, out)) {
        printf("FAIL: d_pred 6 with nb_deltas 0 and no pred plane was refused\n");
        failures++;
    }
    d = good;
    d.bit_depth = 0;
    refusal("bit_depth_0", jxl::palette_check(&d, index, 2, 3, out));
    d.bit_depth = 33;
    refusal("bit_depth_33", jxl::palette_check(&d, index, 2, 3, out));
    d.bit_depth = -8;
    refusal("bit_depth_negative", jxl::palette_check(&d, index, 2, 3, out));
}

static bool read_words(FILE* f, std::vector<int32_t>* v, size_t n) {
    v->resize(n);
    return n == 0 || fread(v->data(), sizeof(int32_t), n, f) == n;
}

int main(int argc, char** argv) {
    refusals();
    int cases = 0;
    if (argc > 2) {
        FILE* in = fopen(argv[1], "rb");
        FILE* res = fopen(argv[2], "wb");
        if (!in || !res) {
            printf("FAIL: cannot open %s or %s\n", argv[1], argv[2]);
            return 2;
        }
        std::vector<int32_t> head, index, palette, pred;
        if (!read_words(in, &head, 1)) return 2;
        const int32_t count = head[0];
        for (; cases < count; cases++) {
            if (!read_words(in, &head, 10)) break;
            const int32_t h = head[0], w = head[1];
            jxl_palette_desc d = {head[2], head[3], head[4], head[5], head[6], head[7], head[8], nullptr, nullptr};
            const size_t n = (size_t)h * w;
            if (!read_words(in, &index, n) || !read_words(in, &palette, (size_t)d.pal_h * d.pal_w) || !read_words(in, &pred, head[9] ? n : 0)) break;
            d.palette = palette.data();
            d.pred = head[9] ? pred.data() : nullptr;
            std::vector<std::vector<int32_t>> planes((size_t)d.num_c, std::vector<int32_t>(n));
            std::vector<int32_t*> out;
            for (auto& p : planes) out.push_back(p.data());
            const char* bad = jxl::palette_check(&d, index.data(), h, w, out.data());
            if (bad) {
                printf("FAIL: case %d refused: %s\n", cases, bad);
                failures++;
                continue;
            }
            const jxl::PaletteLookup lk = {d.palette, d.pal_w, d.nb_colors, d.bit_depth};
            for (int32_t c = 0; c < d.num_c; c++) {
                int32_t* o = out[(size_t)c];
                for (int32_t y = 0; y < h; y++)
                    for (int32_t x = 0; x < w; x++) {
                        const size_t i = (size_t)y * w + x;
                        const int32_t idx = index[i];
                        int32_t v = jxl::palette_value(idx, c, lk);
                        if (idx < d.nb_deltas) {
                            const int32_t p = d.d_pred == 6 ? (d.pred ? jxl::palette_predict_wp(d.pred[i]) : 0)
                                                            : jxl::palette_predict_at(d.d_pred, o, w, x, y);
                            v = jxl::jadd(v, p);
                        }
                        o[i] = v;
                    }
                if (fwrite(o, sizeof(int32_t), n, res) != n) {
                    printf("FAIL: short write\n");
                    return 2;
                }
            }
        }
        if (cases != count) {
            printf("FAIL: the case file is cut short at case %d\n", cases);
            failures++;
        }
        fclose(in);
        fclose(res);
    }
    printf("%d case(s)\n", cases);
    printf("%d failure(s)\n", failures);
    return failures ? 1 : 0;
}
