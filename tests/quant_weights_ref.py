"""A float64 model of the reference's HF quantisation weights (frame/vardct/HFGlobal.java), the second witness for
jxlatte_amd/hfglobal.py: test infrastructure, numpy and math only, nothing imported from jxlatte_amd.

It is written from the Java (file and line beside each piece) and built differently from hfglobal.py: the bands are one cumulative
product, the interpolation is the closed form band[i] * (band[i + 1] / band[i]) ** frac on whole arrays, and nothing is rounded to
float32 -- the only float32 values are the ones the Java source itself holds as float constants or float inputs (the parameters, the
AFV frequencies, SQRT_2 and 1e-6f).

A parameter set is a list of 17 dicts in the shape the decoder hands to hfglobal.generate_weights:
  dict(mode=1..7, dct=[3 lists] | None, par=[3 lists] | None, p44=[3 lists] | None, denominator=float)
tables(params) returns a Tables: the 51 tables in the layout of jxl_vardct_set_weights and, per entry, the K its float32 value is
allowed (see K_OPS / K_DIST) and the "either neighbour" report for a distance that sits within rounding of an integer.

MUTATIONS names deliberately wrong variants of THIS model; tests show that the bound tells each of them from hfglobal.py."""
import math

import numpy as np

D = np.float64
U = 2.0 ** -24  # unit roundoff of float32

MODE_HORNUSS, MODE_DCT2, MODE_DCT4, MODE_DCT4_8, MODE_AFV, MODE_DCT, MODE_RAW = 1, 2, 3, 4, 5, 6, 7  # TransformType.java:39-45
# matrixHeight, matrixWidth of the horizontal type of each parameter index (TransformType.java:10-36, :154-155)
MATRIX = ((8, 8), (8, 8), (8, 8), (8, 8), (16, 16), (32, 32), (8, 16), (8, 32), (16, 32), (8, 8), (8, 8), (64, 64), (32, 64),
          (128, 128), (64, 128), (256, 256), (128, 256))
SMALL = (0, 1, 2, 3, 9, 10)  # TransformType.validateIndex (:59-67): the indexes modes 1..5 may be used on


def legal(index, mode):
    return mode in (MODE_DCT, MODE_RAW) or index in SMALL


MUTATIONS = ("height_for_height_minus_1", "no_1e_6", "len_for_len_minus_1", "linear_interpolation", "afv_2y_2x", "afv_4x8_even_lines",
             "dct4_par_exchanged", "raw_inverted")

# ---- the bound -----------------------------------------------------------------------------------------------------------------
# |w32 - w64| <= K u |w64| per entry, K = K_OPS(i) + K_DIST * pos * |ln(band[i+1] / band[i])|, counted on the longest chain of
# HFGlobal.java:42-77 and :421-431, one u per float32 rounding (products and quotients add their operands' relative errors):
#   band[i]           :61-63   i steps of quantMult (1 - v, then 1 / that: 2) and one product: 3 i
#   b / a             :52      = quantMult (2) and the product's and the quotient's own rounding (2), raised to frac <= 1: 4
#   (float) Math.pow  :52      1 (Math.pow itself is within 1 ulp of the double: 2^-29 u, not counted)
#   a * pow           :52      1
#   /= param          :363-365, :403   1 (DCT4 and DCT4_8 only; counted for all)
#   1.0f / w          :427     1
# so K_OPS(i) = 3 i + 8, at most 3 * 14 + 8 = 50 for the 16 bands four bits can ask for (:31); the last band taken as it is
# (:48-49) has 3 i + 3.
# The position enters through the exponent, where its ABSOLUTE error counts: d(pow) / pow = ln(b / a) * d(frac), and frac = dist -
# (int) dist is exact, so d(frac) = d(dist) = (relative error of dist) * dist. dist (:66-72): the sum and the quotient of `scale` 2,
# y * scale and / (height - 1) 2 more: 4 on dy and on dx; their squares 8 + 1; the sum of two positives 9 + 1; the square root
# halves it: 5; the float cast 1: K_DIST = 6. (The AFV position, :329, has three roundings and is covered by the same 6.)
K_DIST = 6.0
NEAR = 4.0  # a position within NEAR u pos of an integer may fall to either side of it in float32


def k_ops(i):
    return 3.0 * i + 8.0


K_OPS_MAX = k_ops(14)

_F = np.float32
SQRT_2 = float(_F(math.sqrt(2.0)))  # MathHelper.java:8, a float
EPS = float(_F(1e-6))  # HFGlobal.java:66 1e-6f
LOW, HIGH = float(_F(0.8517778890324296)), float(_F(12.97166202570235))  # :307-308


def _f32(v):
    """the float the Java holds for the double `v` (a literal with an f suffix, or a float read from the stream)"""
    return np.asarray(v, D).astype(_F).astype(D)


# HFGlobal.java:19-21
AFV_FREQS = _f32([0, 0, 0.8517778890324296, 5.37778436506804, 0, 0, 4.734747904497923, 5.449245381693219, 1.6598270267479331, 4,
                  7.275749096817861, 10.423227632456525, 2.662932286148962, 7.630657783650829, 8.962388608184032, 12.97166202570235])

# ---- the 17 default sets, transcribed from the text of HFGlobal.java:79-188 (not from hfglobal.DEFAULT_PARAMS) -------------------
_P4X4 = ((2200, 0.0, 0.0, 0.0), (392, 0.0, 0.0, 0.0), (112, -0.25, -0.25, -0.5))  # :96-100
_P4X8 = ((2198.050556016380522, -0.96269623020744692, -0.76194253026666783, -0.6551140670773547),  # :140-144
         (764.3655248643528689, -0.92630200888366945, -0.9675229603596517, -0.27845290869168118),
         (527.107573587542228, -1.4594385811273854, -1.450082094097871593, -1.5843722511996204))
_A = (-1.025, -0.78, -0.65012, -0.19041574084286472, -0.20819395464, -0.421064, -0.32733845535848671)  # :152-153
_B = (-0.3041958212306401, -0.3633036457487539, -0.35660379990111464, -0.3443074455424403, -0.33699592683512467,  # :154-155
      -0.30180866526242109, -0.27321683125358037)
_C = (-1.2, -1.2, -0.8, -0.7, -0.7, -0.4, -0.5)  # :156


def _seq(a, b, c):  # prepend, :23-28
    return ((a,) + _A, (b,) + _B, (c,) + _C)


# (index, mode, dctParam, param, params4x4)
_DEFAULTS = (
    (0, MODE_DCT, ((3150.0, 0.0, -0.4, -0.4, -0.4, -2.0), (560.0, 0.0, -0.3, -0.3, -0.3, -0.3), (512.0, -2.0, -1.0, 0.0, -1.0, -2.0)),  # :81-85
     None, None),
    (1, MODE_HORNUSS, None, ((280.0, 3160.0, 3160.0), (60.0, 864.0, 864.0), (18.0, 200.0, 200.0)), None),  # :86-90
    (2, MODE_DCT2, None, ((3840.0, 2560.0, 1280.0, 640.0, 480.0, 300.0), (960.0, 640.0, 320.0, 180.0, 140.0, 120.0),  # :91-95
                          (640.0, 320.0, 128.0, 64.0, 32.0, 16.0)), None),
    (3, MODE_DCT4, _P4X4, ((1.0, 1.0), (1.0, 1.0), (1.0, 1.0)), _P4X4),  # :101-105
    (4, MODE_DCT, (  # :106-113
        (8996.8725711814115328, -1.3000777393353804, -0.49424529824571225, -0.439093774457103443, -0.6350101832695744,
         -0.90177264050827612, -1.6162099239887414),
        (3191.48366296844234752, -0.67424582104194355, -0.80745813428471001, -0.44925837484843441, -0.35865440981033403,
         -0.31322389111877305, -0.37615025315725483),
        (1157.50408145487200256, -2.0531423165804414, -1.4, -0.50687130033378396, -0.42708730624733904, -1.4856834539296244,
         -4.9209142884401604)), None, None),
    (5, MODE_DCT, (  # :114-120
        (15718.40830982518931456, -1.025, -0.98, -0.9012, -0.4, -0.48819395464, -0.421064, -0.27),
        (7305.7636810695983104, -0.8041958212306401, -0.7633036457487539, -0.55660379990111464, -0.49785304658857626,
         -0.43699592683512467, -0.40180866526242109, -0.27321683125358037),
        (3803.53173721215041536, -3.060733579805728, -2.0413270132490346, -2.0235650159727417, -0.5495389509954993, -0.4, -0.4,
         -0.3)), None, None),
    (6, MODE_DCT, ((7240.7734393502, -0.7, -0.7, -0.2, -0.2, -0.2, -0.5), (1448.15468787004, -0.5, -0.5, -0.5, -0.2, -0.2, -0.2),  # :121-125
                   (506.854140754517, -1.4, -0.2, -0.5, -0.5, -1.5, -3.6)), None, None),
    (7, MODE_DCT, (  # :126-133
        (16283.2494710648897, -1.7812845336559429, -1.6309059012653515, -1.0382179034313539, -0.85, -0.7, -0.9, -1.2360638576849587),
        (5089.15750884921511936, -0.320049391452786891, -0.35362849922161446, -0.30340000000000003, -0.61, -0.5, -0.5, -0.6),
        (3397.77603275308720128, -0.321327362693153371, -0.34507619223117997, -0.70340000000000003, -0.9, -1.0, -1.0,
         -1.1754605576265209)), None, None),
    (8, MODE_DCT, (  # :134-139
        (13844.97076442300573, -0.97113799999999995, -0.658, -0.42026, -0.22712, -0.2206, -0.226, -0.6),
        (4798.964084220744293, -0.61125308982767057, -0.83770786552491361, -0.79014862079498627, -0.2692727459704829,
         -0.38272769465388551, -0.22924222653091453, -0.20719098826199578),
        (1807.236946760964614, -1.2, -1.2, -0.7, -0.7, -0.7, -0.4, -0.5)), None, None),
    (9, MODE_DCT4_8, _P4X8, ((1.0,), (1.0,), (1.0,)), None),  # :145-146
    (10, MODE_AFV, _P4X8, ((3072, 3072, 256, 256, 256, 414, 0.0, 0.0, 0.0), (1024, 1024, 50.0, 50.0, 50.0, 58, 0.0, 0.0, 0.0),  # :147-151
                           (384, 384, 12.0, 12.0, 12.0, 22, -0.25, -0.25, -0.25)), _P4X4),
    (11, MODE_DCT, _seq(23966.1665298448605, 8380.19148390090414, 4493.02378009847706), None, None),  # :157-161
    (12, MODE_DCT, _seq(15358.89804933239925, 5597.360516150652990, 2919.961618960011210), None, None),  # :162-166
    (13, MODE_DCT, _seq(47932.3330596897210, 16760.38296780180828, 8986.04756019695412), None, None),  # :167-171
    (14, MODE_DCT, _seq(30717.796098664792, 11194.72103230130598, 5839.92323792002242), None, None),  # :172-176
    (15, MODE_DCT, _seq(95864.6661193794420, 33520.76593560361656, 17972.09512039390824), None, None),  # :177-181
    (16, MODE_DCT, _seq(61435.5921973295970, 24209.44206460261196, 12979.84647584004484), None, None),  # :182-186
)


def default_params():
    out = []
    for k, (index, mode, dct, par, p44) in enumerate(_DEFAULTS):
        assert k == index
        out.append(dict(mode=mode, dct=None if dct is None else [list(r) for r in dct], par=None if par is None else [list(r) for r in par],
                        p44=None if p44 is None else [list(r) for r in p44], denominator=1.0))
    return out


# ---- the model -----------------------------------------------------------------------------------------------------------------
class Field:
    """values of one interpolated array with what the bound needs: k (per entry), near (the position is within rounding of an
    integer) and other (the value under the other neighbour's band index; the value itself where not near)"""

    def __init__(self, value, k=None, near=None, other=None):
        self.value = np.asarray(value, D)
        self.k = np.full(self.value.shape, 2.0) if k is None else np.asarray(k, D)
        self.near = np.zeros(self.value.shape, bool) if near is None else near
        self.other = self.value.copy() if other is None else np.asarray(other, D)

    def put(self, where, src, pick=None):
        for name in ("value", "k", "near", "other"):
            a = getattr(src, name) if isinstance(src, Field) else None
            if a is None:
                a = {"value": src, "k": 2.0, "near": False, "other": src}[name]
            elif pick is not None:
                a = a[pick]
            getattr(self, name)[where] = a


def bands_of(params):
    """HFGlobal.java:60-64 with quantMult (:55-57) as one cumulative product"""
    p = _f32(params)
    with np.errstate(divide="ignore", invalid="ignore"):
        qm = np.where(p[1:] >= 0, 1.0 + p[1:], 1.0 / (1.0 - np.minimum(p[1:], 0.0)))
    return p[0] * np.concatenate([[1.0], np.cumprod(qm)])


def _at_index(pos, bands, i, linear):
    """interpolate (HFGlobal.java:42-53) with the band index given: i + 1 > len takes the last band as it is"""
    ln = len(bands) - 1
    last = i + 1 > ln
    ic = np.clip(i, 0, ln - 1)
    a, b = bands[ic], bands[ic + 1]
    frac = pos - ic
    with np.errstate(all="ignore"):
        lr = np.log(b / a)
        v = a + (b - a) * frac if linear else a * np.exp(lr * frac)
        k = k_ops(ic) + K_DIST * np.abs(pos * lr)
    return np.where(last, bands[ln], v), np.where(last, 3.0 * ln + 3.0, k)


def interpolate(pos, bands, linear=False, exact=None):
    """`exact`: positions that are the same number in float32 (0 / d and d / d)"""
    pos = np.asarray(pos, D)
    if len(bands) == 1:  # :44-45
        return Field(np.full(pos.shape, bands[0]), np.full(pos.shape, 3.0))
    i = np.floor(pos).astype(np.int64)
    value, k = _at_index(pos, bands, i, linear)
    r = np.rint(pos)
    near = (r >= 1) & (np.abs(pos - r) <= NEAR * U * pos)
    if exact is not None:
        near &= ~exact
    j = np.where(i == r, i - 1, i + 1)
    other, k2 = _at_index(pos, bands, np.maximum(j, 0), linear)
    return Field(value, np.where(near, np.maximum(k, k2), k), near, np.where(near, other, value))


def dct_quant_weights(height, width, params, mut=None):
    """getDCTQuantWeights (HFGlobal.java:59-77)"""
    bands = bands_of(params)
    ln = len(bands) if mut == "len_for_len_minus_1" else len(bands) - 1
    scale = ln / (SQRT_2 + (0.0 if mut == "no_1e_6" else EPS))  # :66
    hd, wd = (height, width) if mut == "height_for_height_minus_1" else (height - 1, width - 1)
    dy = np.arange(height, dtype=D) * scale / hd  # :68
    dx = np.arange(width, dtype=D) * scale / wd  # :71
    return interpolate(np.sqrt(dx[None, :] ** 2 + dy[:, None] ** 2), bands, mut == "linear_interpolation")  # :72-73


def afv_weights(prm, c, mut=None):
    """getAFVTransformWeights (HFGlobal.java:304-345)"""
    w48 = dct_quant_weights(4, 8, prm["dct"][c], mut)
    w44 = dct_quant_weights(4, 4, prm["p44"][c], mut)
    par = _f32(prm["par"][c])
    bands = bands_of(par[5:9])  # :309-317
    w = Field(np.zeros((8, 8)))
    w.put((0, 0), 1.0)  # :319
    for (y, x), v in zip(((1, 0), (0, 1), (2, 0), (0, 2), (2, 2)), par[:5]):  # :320-324
        w.put((y, x), float(v))
    y, x = np.nonzero(~((np.arange(4)[None, :] < 2) & (np.arange(4)[:, None] < 2)))  # :327-328
    freq = AFV_FREQS[y * 4 + x]
    f = interpolate((freq - LOW) / (HIGH - LOW), bands, mut == "linear_interpolation", (freq == LOW) | (freq == HIGH))  # :329
    w.put((2 * y, 2 * x) if mut == "afv_2y_2x" else (2 * x, 2 * y), f)  # :330
    y, x = np.nonzero(np.arange(32).reshape(4, 8) > 0)  # :332-335
    w.put((2 * y + 1, x), w48, (y, x))
    y, x = np.nonzero(np.arange(16).reshape(4, 4) > 0)  # :337-340
    w.put((2 * y, 2 * x + 1), w44, (y, x))
    if mut == "afv_4x8_even_lines":  # the 4 x 8 rows in the even lines, everything else in the odd ones
        swap = np.arange(8) ^ 1
        for name in ("value", "k", "near", "other"):
            setattr(w, name, getattr(w, name)[swap])
    return w


def _spread(f, ry, rx):
    return Field(*(np.repeat(np.repeat(getattr(f, n), ry, 0), rx, 1) for n in ("value", "k", "near", "other")))


def table(index, prm, c, mut=None):
    """the weights of generateWeights (HFGlobal.java:347-420) before the reciprocal"""
    mh, mw = MATRIX[index]
    mode = prm["mode"]
    if mode == MODE_DCT:  # :352-354
        return dct_quant_weights(mh, mw, prm["dct"][c], mut)
    par = _f32(prm["par"][c])
    if mode == MODE_DCT4:  # :355-366
        w = _spread(dct_quant_weights(4, 4, prm["dct"][c], mut), 2, 2)
        p0, p1 = (par[1], par[0]) if mut == "dct4_par_exchanged" else (par[0], par[1])
        with np.errstate(all="ignore"):
            for name in ("value", "other"):
                a = getattr(w, name)
                a[1, 0] /= p0
                a[0, 1] /= p0
                a[1, 1] /= p1
        return w
    if mode == MODE_DCT2:  # :367-385: squares of side 1, 2, 4 along the diagonal and the two blocks beside each
        lvl = np.maximum(np.arange(8)[:, None], np.arange(8)[None, :])
        ring = np.where(lvl < 1, -1, np.where(lvl < 2, 0, np.where(lvl < 4, 1, 2)))
        diag = (np.minimum(np.arange(8)[:, None], np.arange(8)[None, :]) >= np.array([0, 1, 2, 4])[ring + 1])
        v = np.where(ring < 0, 1.0, par[np.maximum(2 * ring + diag, 0)])
        return Field(v)
    if mode == MODE_HORNUSS:  # :386-394
        v = np.full((8, 8), par[0])
        v[1, 1] = par[2]
        v[0, 1] = v[1, 0] = par[1]
        v[0, 0] = 1.0
        return Field(v)
    if mode == MODE_DCT4_8:  # :395-404
        w = _spread(dct_quant_weights(4, 8, prm["dct"][c], mut), 2, 1)
        with np.errstate(all="ignore"):
            w.value[1, 0] /= par[0]
            w.other[1, 0] /= par[0]
        return w
    if mode == MODE_AFV:  # :405-407
        return afv_weights(prm, c, mut)
    if mode == MODE_RAW:  # :408-416: the table TIMES the denominator, and no reciprocal after it (:421)
        v = par.reshape(mh, mw) * float(_F(prm.get("denominator", 1.0)))
        with np.errstate(all="ignore"):
            return Field(1.0 / v if mut == "raw_inverted" else v)
    raise ValueError(mode)


class Tables:
    pass


def tables(params, mut=None):
    """all 51 tables: .w (flat float64), .offs (int[51]), .k, .near, .other (flat, per entry), .valid (bool[17]: every weight of
    a non-RAW set is positive and finite, HFGlobal.java:425-426)"""
    t = Tables()
    t.offs, t.valid = np.zeros(51, np.int64), np.ones(17, bool)
    parts = {n: [] for n in ("value", "k", "near", "other")}
    pos = 0
    for index in range(17):
        for c in range(3):
            f = table(index, params[index], c, mut)
            assert f.value.shape == MATRIX[index]
            if params[index]["mode"] != MODE_RAW:  # :421-431
                if not (np.all(np.isfinite(f.value)) and np.all(f.value > 0)):
                    t.valid[index] = False
                with np.errstate(all="ignore"):
                    f.value, f.other = 1.0 / f.value, 1.0 / f.other
            t.offs[index * 3 + c] = pos
            pos += f.value.size
            for n in parts:
                parts[n].append(getattr(f, n).reshape(-1))
    t.w, t.k, t.near, t.other = (np.concatenate(parts[n]) for n in ("value", "k", "near", "other"))
    return t


def error_ratio(w32, t, lo=0, hi=None):
    """the largest |w32 - w64| / (K u |w64|) over entries lo..hi, every entry under its own K; a near entry is measured against
    the closer of its two values. NaN counts as inf."""
    s = slice(lo, hi)
    got = np.asarray(w32, D)[s]
    with np.errstate(all="ignore"):
        r = np.abs(got - t.w[s]) / (t.k[s] * U * np.abs(t.w[s]))
        r2 = np.abs(got - t.other[s]) / (t.k[s] * U * np.abs(t.other[s]))
    r = np.where(t.near[s], np.minimum(r, r2), r)
    r = np.where(np.isnan(r), np.inf, r)
    return float(r.max()) if r.size else 0.0
