"""The reference's colour-management arithmetic restated for the colour tests (no test in here): TransferFunction.java and
GammaTransferFunction.java with math.pow (glibc) on Python floats where the Java code calls Math.pow on doubles, and
numpy.float32 roundings wherever the Java code rounds to float; MathHelper.max(float...) and the Float.compareTo maximum of
JXLImage.determinePeak as scalar loops. The JVM's pow is unpinned (1 ulp of the double result), as for PQ / sRGB in
csrc/jxl_fastpow.h."""
import math

import numpy as np

F = np.float32
D = np.float64


def _pow1(x, p):
    try:
        return math.pow(x, p)
    except ValueError:      # negative finite base, non-integer exponent: Math.pow gives NaN
        return math.nan
    except OverflowError:
        return math.inf


def jpow(x, p):
    """Math.pow(x, p) per element, p > 0"""
    x = np.asarray(x, D)
    return np.array([_pow1(v, p) for v in x.reshape(-1).tolist()], D).reshape(x.shape)


def to_linear(tf, f, gamma=0, jpow=jpow):
    """TransferFunction.toLinearF; returns (values, on_linear_branch). jpow: the Math.pow stand-in"""
    f = np.asarray(f, F)
    d = f.astype(D)
    with np.errstate(all="ignore"):
        if tf == "linear":
            return f.copy(), np.ones(f.shape, bool)
        if tf == "srgb":  # TransferFunction.java:55-60, float expression into the double pow
            lin = f < F(0.0404482362771082)
            base = ((f * F(0.9478672985781991)).astype(F) + F(0.052132701)).astype(F)
            return np.where(lin, (f * F(0.07739938080495357)).astype(F), jpow(base, 2.4).astype(F)), lin
        if tf == "bt709":  # :73-78
            lin = d < 0.081242858298635133011
            return np.where(lin, (d * 0.22222222222222222222).astype(F),
                            jpow((d + 0.0992968268094429403) * 0.90967241568627260377, 2.2222222222222222222).astype(F)), lin
        if tf == "pq":  # :89-92
            e = jpow(d, 0.012683313515655965121)
            return jpow((e - 0.8359375) / (18.8515625 + 18.6875 * e), 6.2725880551301684533).astype(F), np.zeros(f.shape, bool)
        if tf == "gamma":  # GammaTransferFunction.toLinear
            return jpow(d, 1e7 / gamma).astype(F), np.zeros(f.shape, bool)
    raise KeyError(tf)


def from_linear(tf, f, gamma=0, jpow=jpow):
    """TransferFunction.fromLinearF; returns (values, on_linear_branch)"""
    f = np.asarray(f, F)
    d = f.astype(D)
    with np.errstate(all="ignore"):
        if tf == "bt709":  # :65-70
            lin = d < 0.018053968510807807336
            return np.where(lin, (4.5 * d).astype(F), (1.0992968268094429403 * jpow(d, 0.45) - 0.0992968268094429403).astype(F)), lin
        if tf == "gamma":  # GammaTransferFunction.fromLinear
            return jpow(d, 1e-7 * gamma).astype(F), np.zeros(f.shape, bool)
    raise KeyError(tf)


def cast_to_float(v, max_value):
    """ImageBuffer.castToFloat0 (ImageBuffer.java:112-127)"""
    return (np.asarray(v, np.int32).astype(F) * F(F(1) / F(max_value))).astype(F)


def ulp_distance(a, b):
    """distance in float32 steps (+0 and -0 are one point); NaN lanes must be masked by the caller"""
    def ordered(x):
        i = np.asarray(x, F).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(ordered(a) - ordered(b))


def row_max(a):
    """MathHelper.max(float...) (MathHelper.java:190-195): the minimum, as written"""
    r = a[0]
    for v in a[1:]:
        r = v if v < r else r
    return r


def _compare_to(a, b):
    """Float.compareTo"""
    if a < b:
        return -1
    if a > b:
        return 1
    ia = 0x7FC00000 if a != a else int(F(a).view(np.int32))
    ib = 0x7FC00000 if b != b else int(F(b).view(np.int32))
    return (ia > ib) - (ia < ib)


def determine_peak(plane, int_max=None):
    """JXLImage.determinePeak (:214-223) of one linear plane"""
    if plane.dtype == np.int32:
        return F(F(max(int(v) for v in plane.reshape(-1))) / F(int_max))
    rows = [row_max([F(v) for v in row]) for row in plane]
    best = rows[0]
    for r in rows[1:]:
        if _compare_to(r, best) > 0:
            best = r
    return F(best)
