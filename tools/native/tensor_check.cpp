// Stand-alone host check of jxlatte_amd/csrc/tensor_check.h (no device, no context), meant for an AddressSanitizer + UBSan
// build (tests/test_tensor_cpu.py): the flag rules, the channel and byte counts (64-bit: the largest legal image must not wrap),
// the extent rule of the output pointer and the alignment rule of the kernel's vector stores, over a table of cases.
// Prints "LAYOUT <case> <n_color> <n_out> <elem> <bytes>" per accepted case and ends with "<n> failure(s)".
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <limits>

#include "../../jxlatte_amd/csrc/tensor_check.h"

static int failures = 0;
#define EXPECT(cond, what)                        \
    do {                                          \
        if (!(cond)) {                            \
            printf("FAIL: %s (%s)\n", what, #cond); \
            failures++;                           \
        }                                         \
    } while (0)

static jxl_tensor_params base(int h, int w, int planes, int dtype, int layout) {
    jxl_tensor_params p;
    memset(&p, 0, sizeof p);
    p.color.n_planes = planes;
    p.height = h, p.width = w;
    p.dtype = dtype, p.layout = layout;
    p.alpha_tagged_depth = p.color_tagged_depth = 8;
    for (int c = 0; c < 4; c++) p.inv_std[c] = 1.0f;
    return p;
}

static bool ok(const jxl_tensor_params& p, jxl::TensorLayout* t = nullptr) {
    jxl::TensorLayout mine;
    return jxl::tensor_check_params(&p, t ? t : &mine) == nullptr;
}

static void params() {
    jxl::TensorLayout t;
    jxl_tensor_params p = base(3, 7, 3, JXL_TENSOR_F32, JXL_TENSOR_CHW);
    EXPECT(ok(p, &t) && t.n_color == 3 && t.n_out == 3 && t.elem == 4 && t.pixels == 21 && t.bytes == 252, "RGB f32 3x7");
    printf("LAYOUT rgb_f32 %d %d %d %" PRIu64 "\n", t.n_color, t.n_out, t.elem, t.bytes);
    p = base(3, 7, 1, JXL_TENSOR_U8, JXL_TENSOR_HWC);
    EXPECT(ok(p, &t) && t.n_color == 1 && t.n_out == 1 && t.bytes == 21, "grey u8");
    p.color.use_matrix = 1;
    EXPECT(ok(p, &t) && t.n_color == 3 && t.n_out == 3 && t.bytes == 63, "grey through a matrix: three channels");
    p.has_alpha = p.write_alpha = 1;
    EXPECT(ok(p, &t) && t.n_out == 4 && t.bytes == 84, "and alpha");
    p = base(1, 1, 1, JXL_TENSOR_BF16, JXL_TENSOR_HWC);
    p.has_alpha = p.write_alpha = 1;
    EXPECT(ok(p, &t) && t.n_out == 2 && t.elem == 2 && t.bytes == 4, "grey + alpha bf16");
    printf("LAYOUT ga_bf16 %d %d %d %" PRIu64 "\n", t.n_color, t.n_out, t.elem, t.bytes);
    // the largest sizes the struct can state: no wrap in 64 bits
    p = base(INT32_MAX, INT32_MAX, 3, JXL_TENSOR_F32, JXL_TENSOR_CHW);
    p.has_alpha = p.write_alpha = 1;
    EXPECT(!ok(p), "2^31 - 1 squared at 16 bytes a pixel would wrap: refused");
    p = base(INT32_MAX, INT32_MAX, 1, JXL_TENSOR_U8, JXL_TENSOR_CHW);
    EXPECT(ok(p, &t) && t.pixels == (uint64_t)INT32_MAX * INT32_MAX && t.bytes == t.pixels, "2^31 - 1 squared, one byte a pixel");
    p = base(1 << 30, 1 << 29, 3, JXL_TENSOR_F32, JXL_TENSOR_CHW);
    p.has_alpha = p.write_alpha = 1;
    EXPECT(!ok(p), "2^59 pixels at 16 bytes: 2^63 does not fit");
    p.height = 1 << 29;
    EXPECT(ok(p, &t) && t.bytes == (uint64_t)1 << 62, "2^58 pixels at 16 bytes");
    // refusals
    EXPECT(jxl::tensor_check_params(nullptr, &t) != nullptr, "null params");
    p = base(3, 7, 3, JXL_TENSOR_F32, JXL_TENSOR_CHW);
    EXPECT(jxl::tensor_check_params(&p, nullptr) != nullptr, "null layout");
    p.height = 0;
    EXPECT(!ok(p), "height 0");
    p = base(3, -7, 3, JXL_TENSOR_F32, JXL_TENSOR_CHW);
    EXPECT(!ok(p), "negative width");
    for (int d : {-1, 4, 7, INT32_MAX, INT32_MIN}) {
        p = base(3, 7, 3, d, JXL_TENSOR_CHW);
        EXPECT(!ok(p), "unknown dtype");
    }
    for (int l : {-1, 2, INT32_MAX}) {
        p = base(3, 7, 3, JXL_TENSOR_U8, l);
        EXPECT(!ok(p), "unknown layout");
    }
    p = base(3, 7, 3, JXL_TENSOR_F16, JXL_TENSOR_CHW);
    p.write_alpha = 1;
    EXPECT(!ok(p), "write_alpha without has_alpha");
    p.write_alpha = 0, p.premultiplied = 1;
    EXPECT(!ok(p), "premultiplied without has_alpha");
    p.has_alpha = 1;
    EXPECT(ok(p, &t) && t.n_out == 3, "premultiplied, alpha dropped: still three channels");
    p = base(3, 7, 3, JXL_TENSOR_U8, JXL_TENSOR_CHW);
    p.use_norm = 1;
    EXPECT(!ok(p), "normalisation of U8");
    p.dtype = JXL_TENSOR_F32;
    EXPECT(ok(p), "normalisation of F32");
    p.inv_std[2] = std::numeric_limits<float>::infinity();
    EXPECT(!ok(p), "an infinite inv_std");
    p.inv_std[2] = std::nanf("");
    EXPECT(!ok(p), "a NaN inv_std");
    p.use_norm = 0;
    EXPECT(ok(p), "inv_std is not looked at without use_norm");
    // the depth of an int32 alpha plane, where it is cast
    for (int dtype : {JXL_TENSOR_U8, JXL_TENSOR_F16, JXL_TENSOR_BF16, JXL_TENSOR_F32})
        for (int depth : {0, 32, -3}) {
            p = base(3, 7, 3, dtype, JXL_TENSOR_HWC);
            p.has_alpha = p.write_alpha = p.alpha_is_int = 1;
            p.alpha_tagged_depth = depth;
            EXPECT(!ok(p), "an int alpha plane whose depth has no maximum");
            p.alpha_is_int = 0;
            EXPECT(ok(p), "a float alpha plane has no depth to check");
            p.alpha_is_int = 1, p.write_alpha = 0;
            EXPECT(ok(p), "an alpha plane that is not read is not cast");
        }
    p = base(3, 7, 3, JXL_TENSOR_U8, JXL_TENSOR_HWC);
    p.has_alpha = p.write_alpha = p.alpha_is_int = 1;
    p.alpha_tagged_depth = 8;
    EXPECT(ok(p), "U8, depth 8: clamped as it is");
    p.alpha_tagged_depth = 31;
    EXPECT(ok(p), "depth 31");
    p.alpha_tagged_depth = 1;
    EXPECT(ok(p), "depth 1");
}

static void extents() {
    using jxl::tensor_extent_ok;
    EXPECT(tensor_extent_ok(1000, 100, 1000, 100), "the whole allocation");
    EXPECT(!tensor_extent_ok(1000, 100, 1000, 101), "one byte too many");
    EXPECT(tensor_extent_ok(1000, 100, 1001, 99), "offset by one, one fewer");
    EXPECT(!tensor_extent_ok(1000, 100, 1001, 100), "offset by one, as many");
    EXPECT(!tensor_extent_ok(1000, 100, 999, 1), "in front of the allocation");
    EXPECT(tensor_extent_ok(1000, 100, 1100, 0), "nothing at the end");
    EXPECT(!tensor_extent_ok(1000, 100, 1101, 0), "behind the end");
    EXPECT(!tensor_extent_ok(1000, 100, 1050, UINT64_MAX), "a count that wraps the sum");
    EXPECT(!tensor_extent_ok(UINT64_MAX - 10, 10, UINT64_MAX - 5, 6), "an allocation at the top of the address space");
    EXPECT(tensor_extent_ok(UINT64_MAX - 10, 10, UINT64_MAX - 5, 5), "the same, fitting");
    EXPECT(!tensor_extent_ok(0, 0, 0, 1), "an empty allocation");
}

static void alignment() {
    using jxl::tensor_wide_ok;
    jxl::TensorLayout t;
    jxl_tensor_params p = base(3, 7, 3, JXL_TENSOR_U8, JXL_TENSOR_CHW);
    EXPECT(ok(p, &t), "3x7 RGB u8");
    EXPECT(!tensor_wide_ok(4096, JXL_TENSOR_CHW, t), "CHW, 21 pixels a plane: planes 1 and 2 are misaligned");
    EXPECT(tensor_wide_ok(4096, JXL_TENSOR_HWC, t), "HWC, 12-byte groups on a 4-byte base");
    EXPECT(!tensor_wide_ok(4097, JXL_TENSOR_HWC, t), "HWC offset by one byte");
    p = base(4, 8, 3, JXL_TENSOR_U8, JXL_TENSOR_CHW);
    EXPECT(ok(p, &t) && tensor_wide_ok(4096, JXL_TENSOR_CHW, t) && !tensor_wide_ok(4098, JXL_TENSOR_CHW, t), "CHW u8, 32 pixels");
    p.dtype = JXL_TENSOR_F16;
    EXPECT(ok(p, &t) && tensor_wide_ok(4096, JXL_TENSOR_CHW, t) && tensor_wide_ok(4104, JXL_TENSOR_CHW, t) && !tensor_wide_ok(4100, JXL_TENSOR_CHW, t), "CHW f16: 8-byte stores");
    p.dtype = JXL_TENSOR_F32;
    EXPECT(ok(p, &t) && tensor_wide_ok(4096, JXL_TENSOR_CHW, t) && !tensor_wide_ok(4104, JXL_TENSOR_CHW, t), "CHW f32: 16-byte stores");
    EXPECT(tensor_wide_ok(4096, JXL_TENSOR_HWC, t) && !tensor_wide_ok(4104, JXL_TENSOR_HWC, t), "HWC RGB f32: 48-byte groups, 16-byte stores");
    p = base(3, 7, 1, JXL_TENSOR_F32, JXL_TENSOR_CHW);
    EXPECT(ok(p, &t) && tensor_wide_ok(4096, JXL_TENSOR_CHW, t), "one plane: its size does not matter");
    p = base(3, 7, 1, JXL_TENSOR_F16, JXL_TENSOR_HWC);
    p.has_alpha = p.write_alpha = 1;
    EXPECT(ok(p, &t) && tensor_wide_ok(4096, JXL_TENSOR_HWC, t) && !tensor_wide_ok(4104, JXL_TENSOR_HWC, t), "HWC grey + alpha f16: 16-byte groups");
    // every store unit divides its group: a group's address keeps the base's alignment
    for (int elem : {1, 2, 4})
        for (int nch = 1; nch <= 4; nch++) {
            const int words = nch * elem, unit = jxl::tensor_store_unit(words);
            EXPECT((4 * words) % unit == 0 && unit <= 16 && (unit == 4 || unit == 8 || unit == 16), "HWC store unit");
        }
}

int main() {
    params();
    extents();
    alignment();
    printf("%d failure(s)\n", failures);
    return failures ? 1 : 0;
}
