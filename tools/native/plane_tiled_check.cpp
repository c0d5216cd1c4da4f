// Host-only check of the cell-tiled plane layout (jxlatte_amd/csrc/plane_tiled.h), meant to be built with
// -fsanitize=address,undefined (tests/test_plane_tiled_cpu.py):
//   * plane_tiled_off against the formula of DESIGN.md 2.1 for every (y, x) of a few planes, 72 x 40 among them;
//   * the offsets are a bijection onto [0, W * H): the cells tile the plane without overlap and without holes;
//   * an aligned run of 4 (8) samples is 4 (8) consecutive offsets: 16- and 32-byte accesses stay inside a cell row;
//   * the samples of a cell are the 64 consecutive floats from cell index * 64;
//   * a store pattern like the IDCT launch's (per block: lane = row, float4 pieces) followed by a gather like the restoration
//     kernel's interior loader (per 16-byte piece of every cell a tile overlaps) returns the raster tile, with every access inside
//     the plane's allocation (the buffers are exactly W * H floats: an overrun is an AddressSanitizer report);
//   * plane_tiled_ok refuses planes that are no whole cells or too large for 32-bit sample offsets.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../jxlatte_amd/csrc/plane_tiled.h"

static int failures = 0;
#define CHECK(cond, ...)                          \
    do {                                          \
        if (!(cond)) {                            \
            failures++;                           \
            std::printf("FAIL " __VA_ARGS__);     \
            std::printf("\n");                    \
        }                                         \
    } while (0)

static int64_t formula(int W, int y, int x) { return ((int64_t)(y >> 3) * (W >> 3) + (x >> 3)) * 64 + (y & 7) * 8 + (x & 7); }

static void check_plane(int W, int H) {
    const int cw = W >> 3;
    std::vector<int> seen((size_t)W * H, 0);
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            const uint32_t o = jxl::plane_tiled_off(cw, y, x);
            CHECK((int64_t)o == formula(W, y, x), "%dx%d: off(%d, %d) = %u, formula %lld", W, H, y, x, o, (long long)formula(W, y, x));
            CHECK(o < (uint32_t)(W * H), "%dx%d: off(%d, %d) = %u outside the plane", W, H, y, x, o);
            if (o < (uint32_t)(W * H)) seen[o]++;
            if ((x & 3) == 0)
                for (int i = 1; i < 4; i++) CHECK(jxl::plane_tiled_off(cw, y, x + i) == o + (uint32_t)i, "%dx%d: run of 4 at (%d, %d)", W, H, y, x);
            if ((x & 7) == 0)
                for (int i = 4; i < 8; i++) CHECK(jxl::plane_tiled_off(cw, y, x + i) == o + (uint32_t)i, "%dx%d: run of 8 at (%d, %d)", W, H, y, x);
            CHECK(o / 64 == (uint32_t)((y >> 3) * cw + (x >> 3)), "%dx%d: (%d, %d) outside its cell", W, H, y, x);
        }
    for (size_t i = 0; i < seen.size(); i++) CHECK(seen[i] == 1, "%dx%d: offset %zu hit %d times", W, H, i, seen[i]);

    // write like the IDCT launch (a block's row as 16-byte pieces), read like the restoration kernel's interior tile loader
    std::vector<float> raster((size_t)W * H), tiled((size_t)W * H, -1.0f);
    for (size_t i = 0; i < raster.size(); i++) raster[i] = (float)i;
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x += 4) {
            float* d = tiled.data() + jxl::plane_tiled_off(cw, y, x);
            for (int i = 0; i < 4; i++) d[i] = raster[(size_t)y * W + x + i];
        }
    const int IW = 70, IH = 38;  // the input tile of Gaborish + two EPF iterations
    for (int iy0 = 0; iy0 + IH <= H; iy0 += 3)  // (3 is coprime to 8: every alignment of the tile against the cells)
        for (int ix0 = 0; ix0 + IW <= W; ix0 += 3) {
            std::vector<float> tile((size_t)IW * IH, -2.0f);
            const int NCX = (IW + 6) / 8 + 1, NCY = (IH + 6) / 8 + 1;
            const int ccy0 = iy0 >> 3, ccx0 = ix0 >> 3;
            for (int idx = 0; idx < NCX * NCY * 16; idx++) {
                const int cell = idx >> 4, pc = idx & 15, cyi = cell / NCX, cxi = cell - cyi * NCX;
                const int y = ((ccy0 + cyi) << 3) + (pc >> 1) - iy0, x = ((ccx0 + cxi) << 3) + ((pc & 1) << 2) - ix0;
                if (!((unsigned)y < (unsigned)IH && x > -4 && x < IW)) continue;
                const uint32_t g = ((uint32_t)(ccy0 * cw + ccx0) << 6) + ((uint32_t)(cyi * cw + cxi) << 6) + (uint32_t)(pc << 2);
                const float* s = tiled.data() + g;  // all four samples are read, as the kernel's 16-byte load does
                const float v[4] = {s[0], s[1], s[2], s[3]};
                for (int i = 0; i < 4; i++)
                    if ((unsigned)(x + i) < (unsigned)IW) tile[(size_t)y * IW + x + i] = v[i];
            }
            bool same = true;
            for (int y = 0; y < IH && same; y++)
                for (int x = 0; x < IW && same; x++) same = tile[(size_t)y * IW + x] == raster[(size_t)(iy0 + y) * W + ix0 + x];
            CHECK(same, "%dx%d: tile gathered at (%d, %d) differs from the raster tile", W, H, iy0, ix0);
        }
}

int main() {
    const int sizes[][2] = {{72, 40}, {8, 8}, {64, 32}, {136, 72}, {256, 256}, {80, 48}};
    for (const auto& s : sizes) {
        CHECK(jxl::plane_tiled_ok(s[0], s[1]), "%dx%d refused", s[0], s[1]);
        check_plane(s[0], s[1]);
    }
    CHECK(!jxl::plane_tiled_ok(76, 40), "a width of 76 accepted");
    CHECK(!jxl::plane_tiled_ok(72, 44), "a height of 44 accepted");
    CHECK(!jxl::plane_tiled_ok(0, 8), "an empty plane accepted");
    CHECK(jxl::plane_tiled_ok(32768, 32768), "2^30 samples refused");
    CHECK(!jxl::plane_tiled_ok(65536, 32768), "2^31 samples accepted");
    // the last sample of the largest plane accepted still has a 32-bit offset
    CHECK((int64_t)jxl::plane_tiled_off(65528 >> 3, 32767, 65527) == formula(65528, 32767, 65527), "offset of the last sample of 65528 x 32768");
    std::printf("%d failure(s)\n", failures);
    return failures ? 1 : 0;
}
