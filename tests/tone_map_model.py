"""The expectation of the HDR -> SDR operator, written from its definition and importing nothing of the library:

  * model(): float64 numpy, every constant unrounded -- what the operator means;
  * restated(): the second witness -- the operation order the header's comment documents, type by type: float32 where it says
    float, float64 where it says double, the block's derived constants rounded once to float32;
  * the seeded inputs of the tests, and the mutations a witness must tell apart.

Per pixel, v[3] linear samples in the target primaries:
    Y = lum . v;  ratio = norm where !(Y > 0), max_lum >= 1 or E1 = PQinv(Y unit) / e_src < ks;  else the BT.2408 Annex 5 spline
    (Lb = 0) on E1 clamped to 1, back through PQ, divided by Y unit, times norm;  v *= ratio;  gamut: the least mix toward
    Yo = clamp(Y ratio, 0, 1) that brings every sample into [0, 1].
PQ is SMPTE ST 2084's: c3 enters the denominator of the EOTF with a minus sign."""
import numpy as np

M1, M2, C1, C2, C3 = 0.1593017578125, 78.84375, 0.8359375, 18.8515625, 18.6875
LUM_2020 = (0.2627, 0.6780, 0.0593)  # BT.2020 / BT.2100, D65 (the Y row of its RGB -> XYZ matrix, ITU-R BT.2020 table 4)
LUM_709 = (0.2126, 0.7152, 0.0722)   # BT.709 / sRGB, D65


def pq_inv(L):
    """nits -> signal"""
    p = np.power(np.asarray(L, np.float64) / 10000.0, M1)
    return np.power((C1 + C2 * p) / (1.0 + C3 * p), M2)


def pq(e, mutate=None):
    """signal -> nits"""
    q = np.power(np.asarray(e, np.float64), 1.0 / M2)
    den = C2 + C3 * q if mutate == "pq_plus" else C2 - C3 * q
    return 10000.0 * np.power(np.maximum(q - C1, 0.0) / den, 1.0 / M1)


def constants(unit, source, target):
    e_src = float(pq_inv(source))
    max_lum = float(pq_inv(target)) / e_src
    return e_src, max_lum, 1.5 * max_lum - 0.5, unit / target


def _curve(Y, unit, consts, mutate):
    """the factor of luminance Y (float64 arrays in, float64 out); consts as floats of either precision"""
    e_src, max_lum, ks, norm = [np.float64(c) for c in consts]
    if mutate == "ks_no_half":
        ks = np.float64(1.5) * max_lum
    if max_lum >= 1.0:  # nothing to compress
        return np.ones(Y.shape, np.float64), np.zeros(Y.shape, bool), norm
    with np.errstate(all="ignore"):
        pos = Y > 0
        Ln = np.where(pos, Y, 1.0) * np.float64(unit)
        E1 = pq_inv(Ln) / e_src
        curve = pos & ~(E1 < ks)
        if mutate != "no_clamp":
            E1 = np.minimum(E1, 1.0)
        T = (E1 - ks) / (1.0 - ks)
        T2 = T * T
        T3 = T2 * T
        E2 = (((2.0 * T3 - 3.0 * T2) + 1.0) * ks + ((T3 - 2.0 * T2) + T) * (1.0 - ks)) + (3.0 * T2 - 2.0 * T3) * max_lum
        E2 = np.where(E2 > 0, E2, 0.0)
        Lp = pq(E2 * e_src, mutate)
        return np.where(curve, Lp / Ln, 1.0), curve, norm


def _gamut(v, Yo, dtype, mutate):
    with np.errstate(all="ignore"):
        one, zero = dtype(1), dtype(0)
        Yo = np.where(Yo < 0, zero, np.where(Yo > 1, one, Yo)).astype(dtype)
        toward = np.zeros_like(Yo) if mutate == "gamut_to_zero" else Yo
        t = np.zeros(Yo.shape, dtype)
        for c in range(3):
            den = (v[c] - toward).astype(dtype)
            tc = np.where(v[c] < 0, (v[c] / den).astype(dtype), np.where(v[c] > 1, ((v[c] - one).astype(dtype) / den).astype(dtype), zero))
            t = np.where(tc > t, tc, t)
        t = np.where(t > 1, one, t).astype(dtype)
        out = []
        for c in range(3):
            mixed = (v[c] + (t * (toward - v[c]).astype(dtype)).astype(dtype)).astype(dtype)
            out.append(np.where(t > 0, mixed, v[c]))
    return out


def model(v, lum, unit, source, target, gamut, mutate=None):
    """the operator in float64: v three arrays -> three float64 arrays"""
    v = [np.asarray(a, np.float64) for a in v]
    if mutate == "swap_xb":
        lum = (lum[2], lum[1], lum[0])
    with np.errstate(all="ignore"):
        Y = (lum[0] * v[0] + lum[1] * v[1]) + lum[2] * v[2]
        ratio, curve, norm = _curve(Y, unit, constants(unit, source, target), mutate)
        ratio = np.where(curve, ratio * norm, norm)
        out = [a * ratio for a in v]
        if gamut:
            out = _gamut(out, Y * ratio, np.float64, mutate)
    return out


def restated(v, lum, unit, source, target, gamut):
    """the documented operation order with its types: three float32 arrays"""
    F = np.float32
    v = [np.asarray(a, F) for a in v]
    lum = [F(x) for x in lum]
    consts = [F(c) for c in constants(float(F(unit)), float(F(source)), float(F(target)))]  # rounded once
    with np.errstate(all="ignore"):
        Y = ((lum[0] * v[0]).astype(F) + (lum[1] * v[1]).astype(F)).astype(F) + (lum[2] * v[2]).astype(F)
        Y = Y.astype(F)
        ratio64, curve, _ = _curve(Y.astype(np.float64), float(F(unit)), consts, None)
        norm = consts[3]
        ratio = np.where(curve, (ratio64.astype(F) * norm).astype(F), norm).astype(F)
        out = [(a * ratio).astype(F) for a in v]
        if gamut:
            out = _gamut(out, (Y * ratio).astype(F), F, None)
    return [np.asarray(a, F) for a in out]


def curve64(x, name):
    """the output curve of a linear sample in float64: "linear", "srgb" or "bt709" (the forms of include/jxlatte_amd.h's JXL_TF_*)"""
    x = np.asarray(x, np.float64)
    with np.errstate(all="ignore"):
        if name == "srgb":
            return np.where(x < 0.00313066844250063, x * 12.92, 1.055 * np.power(x, 0.4166666666666667) - 0.055)
        if name == "bt709":
            return np.where(x < 0.018053968510807807336, 4.5 * x, 1.0992968268094429403 * np.power(x, 0.45) - 0.0992968268094429403)
    return x


def curve32(x, name):
    """the same as the colour kernels type it: float32 in and out, the power in float64"""
    F = np.float32
    x = np.asarray(x, F)
    with np.errstate(all="ignore"):
        if name == "srgb":
            p = np.power(x.astype(np.float64), 0.4166666666666667).astype(F)
            return np.where(x < F(0.00313066844250063), (x * F(12.92)).astype(F), ((F(1.055) * p).astype(F) + F(-0.055)).astype(F)).astype(F)
        if name == "bt709":
            d = x.astype(np.float64)
            return np.where(d < 0.018053968510807807336, 4.5 * d, 1.0992968268094429403 * np.power(d, 0.45) - 0.0992968268094429403).astype(F)
    return x


MUTATIONS = ("swap_xb", "ks_no_half", "pq_plus", "no_clamp", "gamut_to_zero")


def knee_luminance(unit, source, target):
    """the linear luminance (in units of `unit` nits) at which E1 == ks"""
    e_src, _, ks, _ = constants(unit, source, target)
    return float(pq(ks * e_src)) / unit


def pixels(h, w, seed, unit=10000.0, source=1000.0, target=203.0, lum=LUM_2020):
    """seeded linear BT.2020 samples up to 1.0 (at `unit` nits a sample), three (h, w) float32 planes: a dark half (the identity
    region), a bright half (the curve, some beyond the source peak), saturated colours (the gamut step), exact zeros, negatives,
    one NaN, and grey pixels a few ulps either side of the knee"""
    rng = np.random.default_rng(seed)
    n = h * w
    peak = source / unit
    mag = np.where(rng.random(n) < 0.5, rng.random(n) * 0.02, rng.random(n)) * np.where(rng.random(n) < 0.7, peak * 1.2, 1.0)
    mag = np.minimum(mag, 1.0)
    v = [(mag * rng.random(n) ** (3.0 * (rng.random(n) < 0.4))).astype(np.float32) for _ in range(3)]
    knee = np.float32(knee_luminance(unit, source, target) / sum(lum))
    special = [(0.0, 0.0, 0.0), (-0.01, 0.2, 0.1), (0.3, -0.02, -0.001), (-0.004, -0.002, -0.01), (np.nan, 0.2, 0.3), (1.0, 1.0, 1.0), (1.0, 0.0, 0.0),
               (0.0, 0.0, 1.0), (peak, peak, peak)]
    for k in (-3, -1, 0, 1, 3):
        g = np.float32(knee)
        for _ in range(abs(k)):
            g = np.nextafter(g, np.float32(2.0 if k > 0 else 0.0), dtype=np.float32)
        special.append((g, g, g))
    at = rng.choice(n, len(special), replace=False)
    for i, px in zip(at, special):
        for c in range(3):
            v[c][i] = np.float32(px[c])
    return [a.reshape(h, w) for a in v]
