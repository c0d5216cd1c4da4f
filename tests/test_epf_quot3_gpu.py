"""epf_quot3 (jxlatte_amd/csrc/epf_quot3.h): the fused restoration kernel's three quotients by one denominator, run on arrays through
the debug hook jxl_debug_epf_quot3, one lane per element. Every result equals numpy's float32 n / d bit for bit (NaNs as NaN).

The helper has two paths behind a wave-uniform branch: inside the window -- every numerator of the element with 2^-100 <= |n| and the
sum of the three magnitudes <= 2^90 -- one refined reciprocal serves the three quotients; one lane outside it sends its whole wave
(64 consecutive elements) to the plain divisions. The cases therefore keep the special numerators uniform over a wave where the
fast path is to be reached, and mix them lane by lane where both kinds are to meet in one wave.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LO = np.float32(2.0 ** -100)
HI = np.float32(2.0 ** 90)
F0, F1, INF = np.float32(0), np.float32(1), np.float32(np.inf)
# the window's two bounds and their neighbours one ulp inside and outside, both signs
HIGH = [HI, np.nextafter(HI, F0), np.nextafter(HI, INF)]
LOW = [LO, np.nextafter(LO, F1), np.nextafter(LO, F0)]
HIGH = np.array(HIGH + [-v for v in HIGH], np.float32)
LOW = np.array(LOW + [-v for v in LOW], np.float32)


def quot3(ctx, n, d):
    """n: [3][count], d: [count] -> [3][count]"""
    fn = ctx.lib.jxl_debug_epf_quot3
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]
    n = np.ascontiguousarray(n, np.float32)
    d = np.ascontiguousarray(d, np.float32)
    assert n.shape == (3, d.size)
    out = np.empty_like(n)
    assert fn(n.ctypes.data, d.ctypes.data, out.ctypes.data, d.size) == 0
    return out


def check(got, n, d, what):
    with np.errstate(all="ignore"):
        exp = n / d[None, :]
    assert exp.dtype == np.float32 and got.dtype == np.float32
    wrong = (got.view(np.uint32) != exp.view(np.uint32)) & ~(np.isnan(got) & np.isnan(exp))
    if wrong.any():
        bad = np.argwhere(wrong)
        raise AssertionError("%s: %d quotients differ; first n = %r, d = %r: got %r, numpy %r" % (
            what, bad.shape[0], n[tuple(bad[0])], d[bad[0][1]], got[tuple(bad[0])], exp[tuple(bad[0])]))


def in_window(rng, count, hi_exp):
    """seeded in-window numerators: either sign, any mantissa, exponent uniform over [2^-100, 2^hi_exp)"""
    bits = rng.integers(0, 1 << 32, count, dtype=np.uint32)
    exps = rng.integers(27, 127 + hi_exp, count, dtype=np.uint32)
    return ((bits & np.uint32(0x807FFFFF)) | (exps << np.uint32(23))).view(np.float32)


@pytest.mark.parametrize("chunk", range(4))
def test_every_denominator_in_1_16(ctx, chunk):
    """every float in [1, 16) -- 2^25 values, 2^23 per case -- against nine numerators each in three calls: a bound or neighbour of the
    upper end, one of the lower end (both uniform over a wave, every pairing of the two occurring) and a seeded in-window value. The
    in-window values stay below 2^60, so that next to the upper bound itself the sum of magnitudes still passes the test."""
    count = 1 << 23
    d = (np.uint32(0x3F800000) + np.uint32(chunk << 23) + np.arange(count, dtype=np.uint32)).view(np.float32)
    assert d[0] == 2.0 ** chunk and d[-1] < 2.0 ** (chunk + 1)
    rng = np.random.default_rng(4100 + chunk)
    wave = np.arange(count) >> 6
    for j in range(3):
        n = np.stack([HIGH[(wave + 2 * j) % 6], LOW[(wave // 6 + 2 * j) % 6], in_window(rng, count, 60)])
        check(quot3(ctx, n, d), n, d, "denominators 2^%d.., call %d" % (chunk, j))


@pytest.mark.parametrize("part", range(4))
def test_random_pairs(ctx, part):
    """2^26 seeded (n, d) pairs with d in [1, 13], 2^24 per case: half of the elements over the whole window, half at the scale of XYB
    samples (the kernel's own numerators)"""
    count = (1 << 24) // 3 + 1
    rng = np.random.default_rng(4200 + part)
    d = (np.float32(1) + np.float32(12) * rng.random(count, dtype=np.float32)).astype(np.float32)
    assert d.min() >= 1 and d.max() <= 13
    wide = np.stack([in_window(rng, count, 88) for _ in range(3)])
    xyb = (rng.standard_normal((3, count)) * np.array([0.02, 0.5, 0.3])[:, None]).astype(np.float32)
    n = np.where((np.arange(count) >> 10 & 1) == 1, wide, xyb).astype(np.float32)
    check(quot3(ctx, n, d), n, d, "random pairs, part %d" % part)


def test_out_of_window_numerators_in_mixed_lanes(ctx):
    """zeros of both signs, denormals, +-2^120, infinities and NaN scattered over the lanes: every wave holds both kinds, and a
    stretch of clean waves follows so that both paths run in one launch"""
    count = 1 << 16
    rng = np.random.default_rng(4300)
    d = (np.float32(1) + np.float32(12) * rng.random(count, dtype=np.float32)).astype(np.float32)
    n = np.stack([in_window(rng, count, 80) for _ in range(3)])
    tiny = np.float32(1e-45)
    odd = np.array([0.0, -0.0, tiny, -tiny, np.float32(1.1e-38), np.float32(-1.1e-38), 2.0 ** 120, -2.0 ** 120, np.inf, -np.inf, np.nan,
                    np.float32(2.0 ** -126), np.finfo(np.float32).max], np.float32)
    hit = rng.random((3, count)) < 0.05
    hit[:, count // 2:] = False  # the second half: clean waves
    n = np.where(hit, odd[rng.integers(0, odd.size, (3, count))], n).astype(np.float32)
    lanes = hit.any(axis=0)[:count // 2].reshape(-1, 64)
    assert lanes.any(axis=1).all() and not lanes.all(axis=1).any()  # every wave of the first half is mixed
    check(quot3(ctx, n, d), n, d, "mixed lanes")
    # the same numerators against denominators at the ends of the range the kernel can produce
    for dv in (1.0, 5.0, 13.0, np.nextafter(np.float32(16), F0)):
        dd = np.full(count, dv, np.float32)
        check(quot3(ctx, n, dd), n, dd, "mixed lanes, d = %r" % dv)
