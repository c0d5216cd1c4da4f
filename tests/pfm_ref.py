"""The independent model of PFMWriter.write (PFMWriter.java:22-49 with ImageBuffer.castToFloat), written from the Java semantics in
numpy. It calls nothing of jxlatte_amd: the tests hold the package's PFM paths against it."""
import numpy as np


def java_depth_max(depth):
    """~(~0 << depth) in Java int arithmetic: 32-bit two's complement, the shift count taken modulo 32"""
    v = ~((0xffffffff << (depth & 31)) & 0xffffffff) & 0xffffffff
    return v - (1 << 32) if v & 0x80000000 else v


def cast(plane, depth):
    """ImageBuffer.castToFloat(depth) of an int plane: (float)v * (1.0f / max), the conversion rounded before the one float
    multiply; a float plane passes through untouched"""
    if plane.dtype == np.float32:
        return plane
    assert plane.dtype == np.int32
    mx = java_depth_max(depth)
    if mx < 1:
        raise ValueError("invalid Max Value")
    scale = np.float32(1.0) / np.float32(mx)
    return plane.astype(np.float32) * scale


def payload(planes, depths=None):
    """the bytes after the header: rows bottom to top, channels interleaved, Float.floatToIntBits, most significant byte first"""
    words = []
    for c, p in enumerate(planes):
        f = np.ascontiguousarray(cast(p, depths[c] if depths is not None else 0), np.float32)
        words.append(np.where(np.isnan(f), np.uint32(0x7fc00000), f.view(np.uint32)))
    return np.stack([w[::-1] for w in words], axis=-1).astype(">u4").tobytes()


def header(n_planes, height, width):
    return ("%s\n%d %d\n1.0\n" % ("Pf" if n_planes == 1 else "PF", width, height)).encode("ascii")


def pfm(planes, depths=None):
    h, w = planes[0].shape
    return header(len(planes), h, w) + payload(planes, depths)
