// Stand-alone host check of jxlatte_amd/csrc/varblock_check.h (no device, no context), meant for an AddressSanitizer + UBSan
// build (tests/test_varblocks_cpu.py):
//   * prints the 27 x 3 tint factors as raw bits ("FACTOR t r g b", hex), for the test to hold against its model
//   * runs the validator over what the entries refuse
//   * with a case file as argv[1] ("cells_h cells_w n" then n rows "cy cx type" per case): builds each cell map, checks it
//     against a walk over the blocks, and prints it ("MAP <case index> <hex bytes>")
// Ends with "<n> failure(s)".
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../jxlatte_amd/csrc/varblock_check.h"

static int failures = 0;
#define EXPECT(cond, what)                        \
    do {                                          \
        if (!(cond)) {                            \
            printf("FAIL: %s (%s)\n", what, #cond); \
            failures++;                           \
        }                                         \
    } while (0)

static const char* run(const std::vector<int32_t>& blocks, int32_t ch, int32_t cw, std::vector<uint8_t>* map) {
    jxl_varblock_desc d;
    d.n_blocks = (int32_t)(blocks.size() / 3);
    d.blocks = blocks.data();  // exactly 3 * n ints: a read past them is the sanitizer's to find
    d.cells_h = ch;
    d.cells_w = cw;
    return jxl::varblock_cell_map(&d, map);
}

static void refusals() {
    std::vector<uint8_t> map;
    EXPECT(run({0, 0, 0}, 1, 1, &map) == nullptr && map.size() == 1 && map[0] == (0 | 0x20 | 0x40), "one DCT8 block");
    EXPECT(run({}, 2, 3, &map) == nullptr && map.size() == 6 && map[5] == 0xff, "an empty list");
    EXPECT(run({0, 0, 27}, 4, 4, &map) != nullptr, "type 27");
    EXPECT(run({0, 0, -1}, 4, 4, &map) != nullptr, "type -1");
    EXPECT(run({0, 0, INT32_MAX}, 4, 4, &map) != nullptr, "type INT32_MAX");
    EXPECT(run({0, 0, 0, 0, 0, 1}, 4, 4, &map) != nullptr, "one cell claimed twice");
    EXPECT(run({0, 0, 4, 1, 1, 0}, 4, 4, &map) != nullptr, "an 8x8 inside a 16x16");
    EXPECT(run({0, 3, 4}, 4, 4, &map) != nullptr, "a 16x16 over the right edge");
    EXPECT(run({3, 0, 4}, 4, 4, &map) != nullptr, "a 16x16 over the bottom edge");
    EXPECT(run({0, 4, 0}, 4, 4, &map) != nullptr, "cx == cells_w");
    EXPECT(run({-1, 0, 0}, 4, 4, &map) != nullptr, "cy < 0");
    EXPECT(run({0, INT32_MAX, 24}, 4, 4, &map) != nullptr, "cx == INT32_MAX");
    EXPECT(run({INT32_MIN, 0, 24}, 4, 4, &map) != nullptr, "cy == INT32_MIN");
    EXPECT(run({0, 0, 24}, 31, 32, &map) != nullptr, "a 256x256 on a 31-row grid");
    EXPECT(run({0, 0, 24}, 32, 32, &map) == nullptr && map.size() == 1024, "a 256x256 that fills its grid");
    EXPECT(run({0, 0, 0}, 0, 4, &map) != nullptr, "no rows");
    EXPECT(run({0, 0, 0}, 4, -1, &map) != nullptr, "negative columns");
    EXPECT(run({}, 65536, 65536, &map) != nullptr, "more cells than INT32_MAX");
    jxl_varblock_desc d = {1, nullptr, 4, 4};
    EXPECT(jxl::varblock_cell_map(&d, &map) != nullptr, "a null list of one block");
    d.n_blocks = -1;
    EXPECT(jxl::varblock_cell_map(&d, &map) != nullptr, "a negative count");
    EXPECT(jxl::varblock_cell_map(nullptr, &map) != nullptr, "a null descriptor");
    d.n_blocks = 0;
    EXPECT(jxl::varblock_cell_map(&d, nullptr) != nullptr, "a null map");
}

// the map against a walk over the blocks that shares nothing with the builder but the type table
static void verify(const std::vector<int32_t>& blocks, int32_t ch, int32_t cw, const std::vector<uint8_t>& map, int index) {
    std::vector<int> owner((size_t)ch * cw, -1);
    size_t owned = 0;
    for (size_t i = 0; i < blocks.size() / 3; i++) {
        const int32_t cy = blocks[3 * i], cx = blocks[3 * i + 1], t = blocks[3 * i + 2];
        for (int y = 0; y < JXL_TT[t].ph / 8; y++)
            for (int x = 0; x < JXL_TT[t].pw / 8; x++) {
                const size_t at = (size_t)(cy + y) * cw + (cx + x);
                EXPECT(owner[at] < 0, "case tiling overlaps");
                owner[at] = (int)i;
                owned++;
                const uint8_t want = (uint8_t)(t | (y == 0 ? 0x20 : 0) | (x == 0 ? 0x40 : 0));
                if (map[at] != want) {
                    printf("FAIL: case %d cell (%d, %d): %02x, expected %02x\n", index, cy + y, cx + x, map[at], want);
                    failures++;
                }
            }
    }
    size_t free_cells = 0;
    for (size_t at = 0; at < map.size(); at++)
        if (owner[at] < 0) {
            free_cells++;
            EXPECT(map[at] == 0xff, "an unowned cell is 0xFF");
        }
    EXPECT(owned + free_cells == map.size(), "every cell counted once");
}

int main(int argc, char** argv) {
    float f[jxl::kVbTypes * 3];
    jxl::varblock_factors(f);
    for (int t = 0; t < jxl::kVbTypes; t++) {
        uint32_t b[3];
        memcpy(b, f + 3 * t, sizeof b);
        printf("FACTOR %d %08" PRIx32 " %08" PRIx32 " %08" PRIx32 "\n", t, b[0], b[1], b[2]);
    }
    refusals();
    if (argc > 1) {
        FILE* in = fopen(argv[1], "r");
        if (!in) {
            printf("FAIL: cannot open %s\n", argv[1]);
            return 2;
        }
        int ch, cw, n, index = 0;
        while (fscanf(in, "%d %d %d", &ch, &cw, &n) == 3) {
            std::vector<int32_t> blocks((size_t)3 * n);
            for (size_t i = 0; i < blocks.size(); i++)
                if (fscanf(in, "%" SCNd32, &blocks[i]) != 1) {
                    printf("FAIL: case %d is cut short\n", index);
                    fclose(in);
                    return 2;
                }
            std::vector<uint8_t> map;
            const char* bad = run(blocks, ch, cw, &map);
            if (bad) {
                printf("FAIL: case %d refused: %s\n", index, bad);
                failures++;
            } else {
                verify(blocks, ch, cw, map, index);
                std::string hex;
                char two[3];
                for (uint8_t m : map) {
                    snprintf(two, sizeof two, "%02x", m);
                    hex += two;
                }
                printf("MAP %d %s\n", index, hex.c_str());
            }
            index++;
        }
        fclose(in);
        printf("%d case(s)\n", index);
    }
    printf("%d failure(s)\n", failures);
    return failures ? 1 : 0;
}
