// The pure part of the tensor entries' checks (tensor_host.hip): the flag rules, the channel count, the byte count in 64-bit
// arithmetic, the extent rule of the output pointer and the alignment rule of the kernel's vector stores. Plain C++: no device
// call, no context; tools/native/tensor_check.cpp runs it as a program of its own under the sanitizers. What jxl_png_params
// shares with jxl_tensor_params (sizes, the colour stages, the alpha plane) is checked by the PNG entries' own code.
#ifndef JXL_TENSOR_CHECK_H
#define JXL_TENSOR_CHECK_H
#include <cmath>
#include <stdint.h>

#include "../../include/jxlatte_amd.h"

namespace jxl {

struct TensorLayout {
    int n_color;       // 3 when color.n_planes == 3, color.use_matrix or the context's tone mapping is armed, else 1
    int n_out;         // + 1 when alpha is written
    int elem;          // bytes of one element
    uint64_t pixels;   // height * width
    uint64_t bytes;    // pixels * n_out * elem
};

inline int tensor_elem_bytes(int32_t dtype) {
    return dtype == JXL_TENSOR_U8 ? 1 : (dtype == JXL_TENSOR_F16 || dtype == JXL_TENSOR_BF16) ? 2 : dtype == JXL_TENSOR_F32 ? 4 : 0;
}

// nullptr, or why the parameters are refused; *out is filled when they are not. tone_map: the context's tone mapping is armed
// (jxl_ctx_set_tone_map), which makes three colour channels as use_matrix does
inline const char* tensor_check_params(const jxl_tensor_params* p, TensorLayout* out, bool tone_map = false) {
    if (!p || !out) return "tensor samples: null argument";
    if (p->height <= 0 || p->width <= 0) return "tensor samples: bad size";
    const int elem = tensor_elem_bytes(p->dtype);
    if (!elem) return "tensor samples: unknown dtype";
    if (p->layout != JXL_TENSOR_CHW && p->layout != JXL_TENSOR_HWC) return "tensor samples: unknown layout";
    if ((p->write_alpha || p->premultiplied) && !p->has_alpha) return "tensor samples: write_alpha and premultiplied need an alpha plane";
    if (p->use_norm) {
        if (p->dtype == JXL_TENSOR_U8) return "tensor samples: normalisation is for the float dtypes";
        for (int c = 0; c < 4; c++)
            if (!std::isfinite(p->inv_std[c])) return "tensor samples: inv_std is not finite";
    }
    // where the alpha plane is cast: always for the float dtypes; for U8 where PNGWriter coerces (premultiplied, or a depth other than 8)
    const bool alpha_read = p->has_alpha && (p->write_alpha || p->premultiplied);
    const bool cast = p->dtype != JXL_TENSOR_U8 || p->premultiplied || p->alpha_tagged_depth != 8;
    if (alpha_read && p->alpha_is_int && cast && (p->alpha_tagged_depth < 1 || p->alpha_tagged_depth > 31)) return "invalid Max Value";
    out->n_color = (p->color.n_planes == 3 || p->color.use_matrix || tone_map) ? 3 : 1;
    out->n_out = out->n_color + (p->write_alpha ? 1 : 0);
    out->elem = elem;
    out->pixels = (uint64_t)p->height * (uint64_t)p->width;  // < 2^62: no wrap
    const uint64_t pixel_bytes = (uint64_t)(out->n_out * out->elem);  // at most 16
    if (out->pixels > (uint64_t)INT64_MAX / pixel_bytes) return "tensor samples: the tensor's size does not fit 63 bits";
    out->bytes = out->pixels * pixel_bytes;
    return nullptr;
}

// the allocation [base, base + range) holds [ptr, ptr + needed)
inline bool tensor_extent_ok(uint64_t base, uint64_t range, uint64_t ptr, uint64_t needed) {
    if (ptr < base) return false;
    const uint64_t off = ptr - base;
    return off <= range && needed <= range - off;
}

// the widest store of a group of `words` words (tensor_store.h: store_words)
inline int tensor_store_unit(int words) { return words % 4 == 0 ? 16 : words % 2 == 0 ? 8 : 4; }

// every full group of 4 pixels may leave in the kernel's vector stores: each group's address has its store's alignment
inline bool tensor_wide_ok(uint64_t ptr, int32_t layout, const TensorLayout& t) {
    if (layout == JXL_TENSOR_HWC) return ptr % (uint64_t)tensor_store_unit(t.n_out * t.elem) == 0;
    const uint64_t unit = (uint64_t)tensor_store_unit(t.elem);  // a channel's 4 elements: 4 * elem bytes, one store
    return ptr % unit == 0 && (t.n_out == 1 || t.pixels % 4 == 0);
}

}  // namespace jxl
#endif  // JXL_TENSOR_CHECK_H
