"""numpy model of what the tensor exit adds on top of float planes: un-premultiplication, normalisation, the rounding to float16 /
bfloat16 and the layout. Nothing else: the colour stages, the alpha cast and the U8 quantiser are pinned against the library's
own earlier entries (jxl_stage_color_convert, jxl_stage_png_samples) by the tests that use this module."""
import numpy as np

F = np.float32
F16_NAN, BF16_NAN = 0x7E00, 0x7FC0


def f32(bits):
    """float32 array from uint32 bit patterns"""
    return np.asarray(bits, np.uint32).view(F)


def to_bf16_bits(x):
    """round to nearest even from the f32; overflow goes to infinity; every NaN is BF16_NAN. uint16 bit patterns"""
    u = np.ascontiguousarray(x, F).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    return np.where(np.isnan(x), np.uint16(BF16_NAN), r)


def to_f16_bits(x):
    """round to nearest even from the f32 in integer arithmetic (not numpy's cast): subnormals kept, overflow to infinity, every
    NaN F16_NAN. uint16 bit patterns"""
    x = np.ascontiguousarray(x, F)
    u = x.view(np.uint32).astype(np.int64)
    sign = ((u >> 16) & 0x8000).astype(np.int64)
    mag = u & 0x7FFFFFFF
    e = (mag >> 23) - 127  # unbiased
    m = (mag & 0x7FFFFF) | 0x800000  # 24-bit significand of a normal f32
    # f16 normal: e in [-14, 15], 10 fraction bits: drop 13; subnormal (e < -14): drop 13 + (-14 - e), no more than 25 (all gone)
    drop = np.where(e < -14, np.minimum(13 + (-14 - e), 25), 13)
    m = np.where(mag < 0x00800000, 0, m)  # f32 zeros and subnormals are far below half the least f16 subnormal
    kept = m >> drop
    rem = m & ((np.int64(1) << drop) - 1)
    half = np.int64(1) << (drop - 1)
    kept = kept + ((rem > half) | ((rem == half) & ((kept & 1) == 1)))
    # kept: the 11-bit significand (hidden bit at 0x400) of a normal, or the fraction of a subnormal; a carry moves it up by itself
    normal = (np.maximum(e, -14) + 14).astype(np.int64) << 10  # biased exponent - 1, added to a significand WITH its hidden bit
    bits = np.where(e < -14, kept, normal + kept)
    bits = np.where(bits >= 0x7C00, 0x7C00, bits)  # overflow (f32 infinity included: e = 128)
    out = (sign | bits).astype(np.uint16)
    return np.where(np.isnan(x), np.uint16(F16_NAN), out)


def unpremultiply(colors, alpha):
    """colour / alpha, the f32 division, per plane"""
    with np.errstate(all="ignore"):
        return [(c / alpha).astype(F) for c in colors]


def normalise(planes, mean, inv_std):
    """(v - mean[c]) * inv_std[c], each operation rounded to f32"""
    with np.errstate(all="ignore"):
        return [((p - F(mean[c])).astype(F) * F(inv_std[c])).astype(F) for c, p in enumerate(planes)]


def convert(planes, dtype):
    """planes (float32) as the element bit patterns of dtype: 'float32' uint32, 'float16' / 'bfloat16' uint16"""
    if dtype == "float32":
        return [np.ascontiguousarray(p, F).view(np.uint32) for p in planes]
    return [to_f16_bits(p) if dtype == "float16" else to_bf16_bits(p) for p in planes]


def layout(planes, which):
    """[C][H][W] for 'CHW', [H][W][C] for 'HWC'"""
    a = np.stack(planes)
    return a if which == "CHW" else np.ascontiguousarray(np.moveaxis(a, 0, -1))
