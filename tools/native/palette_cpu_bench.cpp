// The front-end's own inverse Palette loop (ModularStream::apply_transforms, jxlatte_amd/frontend/modular.cc) timed on the inputs
// of tools/palette_bench.py: a measurement harness, not product. Built from this file plus the front-end's modular.cc and
// entropy.cc (tools/palette_bench.py has the command).
//   palette_cpu_bench <case file> [rounds]
// The case file has the layout of tools/native/palette_check.cpp. Each case becomes a stream of two channels (the palette, the
// index plane) with one Palette transform; every round rebuilds the stream and times apply_transforms alone. Prints
// "CASE <i> <best ms> <median ms> <checksum>" per case. The stream's bit depth is the front-end's default, 8: cases of another
// depth are refused.
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../jxlatte_amd/frontend/modular.h"

static bool read_words(FILE* f, std::vector<int32_t>* v, size_t n) {
    v->resize(n);
    return n == 0 || fread(v->data(), sizeof(int32_t), n, f) == n;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const int rounds = argc > 2 ? std::max(1, atoi(argv[2])) : 5;
    FILE* in = fopen(argv[1], "rb");
    if (!in) return 2;
    std::vector<int32_t> head, index, palette, pred;
    if (!read_words(in, &head, 1)) return 2;
    const int32_t count = head[0];
    for (int32_t i = 0; i < count; i++) {
        if (!read_words(in, &head, 10)) return 2;
        const int32_t h = head[0], w = head[1], pal_h = head[7], pal_w = head[8];
        if (!read_words(in, &index, (size_t)h * w) || !read_words(in, &palette, (size_t)pal_h * pal_w) || !read_words(in, &pred, head[9] ? (size_t)h * w : 0))
            return 2;
        if (head[6] != 8) {
            printf("CASE %d refused: bit depth %d\n", i, head[6]);
            continue;
        }
        std::vector<double> ms;
        uint32_t sum = 0;
        for (int r = 0; r < rounds; r++) {
            jxf::ModularStream s;
            jxf::Channel pal(pal_h, pal_w, 0, 0), idx(h, w, 0, 0);
            pal.buf = palette;
            idx.buf = index;
            idx.pred = pred;
            s.channels = {pal, idx};
            jxf::Transform t;
            t.tr = jxf::Transform::kPalette;
            t.begin_c = 0;
            t.num_c = head[2];
            t.nb_colors = head[3];
            t.nb_deltas = head[4];
            t.d_pred = head[5];
            s.transforms = {t};
            s.nb_meta = 1;
            s.empty = false;
            const auto t0 = std::chrono::steady_clock::now();
            s.apply_transforms(nullptr);
            const auto t1 = std::chrono::steady_clock::now();
            ms.push_back(std::chrono::duration<double, std::milli>(t1 - t0).count());
            sum = 0;
            for (const jxf::Channel& c : s.channels)
                for (int32_t v : c.buf) sum = sum * 31u + (uint32_t)v;
        }
        std::sort(ms.begin(), ms.end());
        printf("CASE %d %.3f %.3f %08x\n", i, ms.front(), ms[ms.size() / 2], sum);
    }
    fclose(in);
    return 0;
}
