// What the tensor kernels (k_tensor.hip, k_tensor_resize.hip) share behind their arithmetic: the conversion of an f32 to the
// element's bits, and the element and word stores.
#ifndef JXL_TENSOR_STORE_H
#define JXL_TENSOR_STORE_H
#include "jxl_internal.h"

namespace jxl {
namespace {

// f32 -> the element's bits (below 2^(8 BYTES) for the narrow dtypes)
template <int BYTES>
__device__ __forceinline__ uint32_t tensor_float_bits(float v, int dtype) {
    const uint32_t u = __builtin_bit_cast(uint32_t, v);
    if (BYTES == 4) return u;
    if (v != v) return dtype == JXL_TENSOR_BF16 ? 0x7FC0u : 0x7E00u;
    if (dtype == JXL_TENSOR_BF16) return (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;  // (no carry out of a finite or infinite f32)
    return (uint32_t)__builtin_bit_cast(uint16_t, (_Float16)v);  // v_cvt_f16_f32: nearest even, subnormals kept, overflow to inf
}

// element e of a register file that holds consecutive BYTES-wide elements
template <int BYTES>
__device__ __forceinline__ void store_element(void* out, int64_t at, const uint32_t* reg, int e) {
    const uint32_t word = reg[(e * BYTES) >> 2] >> (8 * ((e * BYTES) & 3));
    if (BYTES == 1) ((uint8_t*)out)[at] = (uint8_t)word;
    else if (BYTES == 2) ((uint16_t*)out)[at] = (uint16_t)word;
    else ((uint32_t*)out)[at] = word;
}

// WORDS consecutive words to a WORDS * 4-byte group whose address is aligned to min(16, the largest power of two in WORDS * 4)
template <int WORDS>
__device__ __forceinline__ void store_words(uint32_t* o, const uint32_t* reg) {
    if constexpr (WORDS % 4 == 0) {
#pragma unroll
        for (int j = 0; j < WORDS; j += 4) *reinterpret_cast<uint4*>(o + j) = make_uint4(reg[j], reg[j + 1], reg[j + 2], reg[j + 3]);
    } else if constexpr (WORDS % 2 == 0) {
#pragma unroll
        for (int j = 0; j < WORDS; j += 2) *reinterpret_cast<uint2*>(o + j) = make_uint2(reg[j], reg[j + 1]);
    } else {  // 4 or 12 bytes: adjacent dword stores (hipcc joins the three into a global_store_dwordx3, as in k_png_samples)
#pragma unroll
        for (int j = 0; j < WORDS; j++) o[j] = reg[j];
    }
}

}  // namespace
}  // namespace jxl
#endif  // JXL_TENSOR_STORE_H
