"""A second model of the stages outside the VarDCT pixel path, restated for the tests (no test in here): the LF stage, k-times
upsampling, noise synthesis, modularToFloat and the Modular transforms (tendency, the inverse Squeeze steps, all 42 RCT types, the
squeeze / RCT part of applyTransforms).

Like tests/vardct_ref64.py it is a second witness next to oracle/ (a line-by-line C restatement that the kernels are compared with
bit for bit): written from the reference's Java in whole-array numpy, in its own formulation, importing nothing of this project.

Float stages are computed in float64 from float32 inputs taken as exact; where a stage is linear its result comes with the MAGNITUDE
COMPANION A (the same computation on absolute values), and the tests bound |float32 result - model| by K u (A + |model|), u = 2^-24.
Integer stages are computed in int64 arrays holding int32 values, with Java's semantics made explicit: wrap after every operation
(_add, _sub, _mul), `/` truncating toward zero (_tdiv), `>>` arithmetic. The noise generator runs in uint64 arrays (which wrap).

`mut=` selects deliberately WRONG variants (the mutation table of tests/test_pixel_ref64_cpu.py); production comparisons pass none.
Citations are file:line of the reference (java/com/traneptora/jxlatte/...)."""
import numpy as np

D = np.float64
F = np.float32
U = 2.0 ** -24  # unit roundoff of float32

MUTATIONS = ("lf_cfl_127", "lf_gap_divided_sd", "lf_gap_per_channel", "lf_weights_exchanged", "up_max_neg_max", "up_kykx_exchanged",
             "noise_seed_xy_exchanged", "noise_batch_high_low", "noise_colour_innermost", "noise_corr_exchanged", "rct_perm_inverse",
             "tend_div12_floor", "squeeze_half_floor", "squeeze_next_avg_zero")


def _mut(mut, name):
    if mut is not None and mut not in MUTATIONS:
        raise KeyError(mut)
    return mut == name


def f32(v):
    """a float32 value (or array of them) as an exact float64"""
    return np.asarray(np.asarray(v, F), D)


def error_ratio(got, model, companion):
    """the largest |got - model| / (u (A + |model|)): the K a result needs. Where the bound is 0 the result must be exact (inf
    otherwise); NaN in either counts as inf."""
    got, model, companion = np.asarray(got, D), np.asarray(model, D), np.asarray(companion, D)
    err = np.abs(got - model)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / (U * (companion + np.abs(model))))
    r = np.where(np.isnan(r), np.inf, r)
    return float(r.max()) if r.size else 0.0


def mirror(c, n):
    """MathHelper.mirrorCoordinate (util/MathHelper.java:323-329) in closed form: the reflections repeat with period 2n"""
    m = np.mod(c, 2 * n)
    return np.where(m < n, m, 2 * n - 1 - m)


def _windows(p):
    """the 5 x 5 neighbourhood of every sample on mirrored coordinates: [iy][ix][y][x]"""
    h, w = p.shape
    ys = mirror(np.arange(-2, h + 2), h)
    xs = mirror(np.arange(-2, w + 2), w)
    pad = p[np.ix_(ys, xs)]
    return np.stack([np.stack([pad[iy:iy + h, ix:ix + w] for ix in range(5)]) for iy in range(5)])


# ---- LF stage (frame/vardct/LFCoefficients.java:64-100, 113-180) ----------------------------------------------------------------
LF_W = (0.05226273532324128, 0.20345139757231578, 0.0334829185968739)  # :139-140: centre, adjacent, diagonal (float literals)


def lf_stage(q, scaled_dequant, extra_precision=0, x_factor_lf=128, b_factor_lf=128, smooth=True, base_corr_x=0.0,
             base_corr_b=1.0, color_factor=84, mut=None):
    """q: int [3][H][W] in X, Y, B order. Returns (planes, A, gap): gap is the per-cell value BEFORE max(0, 3 - 4 g) (:152), shape
    (H - 2, W - 2), or None where nothing is smoothed."""
    q = np.asarray(q).astype(D)
    sd_full = f32(scaled_dequant)
    sd = sd_full / float(1 << extra_precision)                                      # :68, a power of two: exact
    d = q * sd[:, None, None]                                                       # :73
    ad = np.abs(d)
    off = 127.0 if _mut(mut, "lf_cfl_127") else 128.0
    x, a = d.copy(), ad.copy()
    for c, base, fac in ((0, base_corr_x, x_factor_lf), (2, base_corr_b, b_factor_lf)):  # :80-93
        k = float(f32(base)) + (fac - off) / float(color_factor)
        ak = abs(float(f32(base))) + abs(fac - off) / float(color_factor)
        x[c] = d[c] + k * d[1]
        a[c] = ad[c] + ak * ad[1]
    if not smooth or min(q.shape[1:]) < 3:
        return x, a, None
    w0, w1, w2 = (float(f32(v)) for v in LF_W)
    if _mut(mut, "lf_weights_exchanged"):
        w1, w2 = w2, w1

    def weighted(c):
        ctr = c[:, 1:-1, 1:-1]
        adj = c[:, 1:-1, :-2] + c[:, 1:-1, 2:] + c[:, :-2, 1:-1] + c[:, 2:, 1:-1]
        dia = c[:, :-2, :-2] + c[:, :-2, 2:] + c[:, 2:, :-2] + c[:, 2:, 2:]
        return ctr, w0 * ctr + w1 * adj + w2 * dia                                  # :135-140
    ctr, wgt = weighted(x)
    actr, awgt = weighted(a)
    gsd = sd if _mut(mut, "lf_gap_divided_sd") else sd_full                         # :120: scaledDequant[i], undivided
    g = np.abs(ctr - wgt) * gsd[:, None, None]                                      # :141
    shared = np.maximum(0.5, g.max(axis=0))                                         # :127, :142-143: one gap for the three channels
    gap = np.maximum(0.5, g) if _mut(mut, "lf_gap_per_channel") else shared[None]
    fac = np.maximum(0.0, 3.0 - 4.0 * gap)                                          # :152
    out, aout = x.copy(), a.copy()                                                  # :165-172: the border is copied
    out[:, 1:-1, 1:-1] = (ctr - wgt) * fac + wgt                                    # :174
    aout[:, 1:-1, 1:-1] = (actr + awgt) * fac + awgt
    return out, aout, shared


def lf_regimes(gap):
    """shares of the interior cells with gap = 0.5 (factor 1), 0.5 < gap < 0.75, gap >= 0.75 (factor 0)"""
    return float((gap == 0.5).mean()), float(((gap > 0.5) & (gap < 0.75)).mean()), float((gap >= 0.75).mean())


# ---- k-times upsampling (frame/Frame.java:217-260, bundle/ImageHeader.java:441-470) ------------------------------------------
def up_weights(k, packed):
    """[k][k][5][5] from the 15 / 55 / 210 packed coefficients. ImageHeader.java:458-462 indexes the upper triangle (row-major,
    index = N y - y (y - 1) / 2 + x - y, N = 5k/2) of a symmetric N x N matrix through (i, j) sorted, and mirrors the second half of
    either axis (4 - iy + 5 (k - 1 - ky) is 5k - 1 - (5 ky + iy)): the table is that matrix continued symmetrically to 5k x 5k and
    cut into 5 x 5 tiles."""
    n = 5 * k // 2
    packed = f32(packed)
    assert packed.size == n * (n + 1) // 2
    s = np.zeros((n, n), D)
    s[np.triu_indices(n)] = packed
    s = s + np.triu(s, 1).T
    full = np.block([[s, s[:, ::-1]], [s[::-1, :], s[::-1, ::-1]]])
    return full.reshape(k, 5, k, 5).transpose(0, 2, 1, 3)


FLOAT_MIN_VALUE = 2.0 ** -149  # Float.MIN_VALUE: the smallest POSITIVE float (Frame.java:241 starts max there)
FLOAT_MAX_VALUE = float(np.finfo(F).max)


def upsample(plane, k, weights, mut=None):
    """weights: [k][k][5][5] (float32 values). Returns (out, A, clamped): clamped marks outputs replaced by the window's min / max"""
    p = f32(plane)
    wt = f32(weights)
    if _mut(mut, "up_kykx_exchanged"):
        wt = wt.transpose(1, 0, 2, 3)
    h, w = p.shape
    win = _windows(p)
    total = np.einsum("abij,ijyx->yaxb", wt, win).reshape(h * k, w * k)             # :251
    a = np.einsum("abij,ijyx->yaxb", np.abs(wt), np.abs(win)).reshape(h * k, w * k)
    lo = np.minimum(win.min(axis=(0, 1)), FLOAT_MAX_VALUE)                          # :240, :247-248
    hi = np.maximum(win.max(axis=(0, 1)), -FLOAT_MAX_VALUE if _mut(mut, "up_max_neg_max") else FLOAT_MIN_VALUE)  # :241, :249-250
    lo, hi = (np.repeat(np.repeat(v, k, 0), k, 1) for v in (lo, hi))
    out = np.where(total < lo, lo, np.where(total > hi, hi, total))                 # :254
    return out, a, out != total


# ---- noise (frame/Frame.java:748-834, frame/features/XorShiro.java) -------------------------------------------------------------
_GOLDEN = np.uint64(0x9e3779b97f4a7c15)


def split_mix64(z):
    """XorShiro.java:9-13 on uint64 arrays (products wrap)"""
    z = np.asarray(z, np.uint64)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xbf58476d1ce4e5b9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94d049bb133111eb)
    return z ^ (z >> np.uint64(31))


def xorshiro_batches(seed0, seed1, count, mut=None):
    """seed1: uint64 [G], one generator per entry. Returns uint32 [G][count][16]: `count` batches of each generator (:49-61), all
    generators advanced together"""
    seed1 = np.asarray(seed1, np.uint64)
    g = seed1.size
    s0 = np.empty((g, 8), np.uint64)
    s1 = np.empty((g, 8), np.uint64)
    s0[:, 0] = split_mix64(np.full(g, seed0 & 0xFFFFFFFFFFFFFFFF, np.uint64) + _GOLDEN)   # :26-31
    s1[:, 0] = split_mix64(seed1 + _GOLDEN)
    for i in range(1, 8):
        s0[:, i] = split_mix64(s0[:, i - 1])
        s1[:, i] = split_mix64(s1[:, i - 1])
    out = np.empty((g, count, 8, 2), np.uint32)
    lo_first = not _mut(mut, "noise_batch_high_low")
    for t in range(count):
        a, b = s1, s0
        c = a + b
        s0 = a
        b = b ^ (b << np.uint64(23))
        s1 = b ^ a ^ (b >> np.uint64(18)) ^ (a >> np.uint64(5))
        low, high = (c & np.uint64(0xFFFFFFFF)).astype(np.uint32), (c >> np.uint64(32)).astype(np.uint32)
        out[:, t, :, 0] = low if lo_first else high                                # :57-58
        out[:, t, :, 1] = high if lo_first else low
    return out.reshape(g, count, 16)


def noise_local(h, w, seed0, group_dim=256, colors=3, mut=None):
    """the local samples of Frame.java:752-773 as uint32 bit patterns [colors][h][w] (floats in [1, 2))"""
    gy, gx = -(-h // group_dim), -(-w // group_dim)
    y0 = (np.arange(gy * gx) // gx) * group_dim
    x0 = (np.arange(gy * gx) % gx) * group_dim
    hi, lo = (y0, x0) if _mut(mut, "noise_seed_xy_exchanged") else (x0, y0)
    seed1 = (hi.astype(np.uint64) << np.uint64(32)) | lo.astype(np.uint64)          # :757
    ys = np.minimum(group_dim, h - y0)
    xs = np.minimum(group_dim, w - x0)
    runs = -(-xs // 16)                                                             # :764-766: a truncated run still takes a batch
    bits = xorshiro_batches(seed0, seed1, int((colors * ys * runs).max()), mut)
    out = np.zeros((colors, h, w), np.uint32)
    for g in range(gy * gx):
        n = int(colors * ys[g] * runs[g])
        b = bits[g, :n]
        if _mut(mut, "noise_colour_innermost"):
            b = b.reshape(ys[g], runs[g], colors, 16).transpose(2, 0, 1, 3)
        b = b.reshape(colors, ys[g], runs[g] * 16)[:, :, :xs[g]]                    # :762-764: colour, row, run
        out[:, y0[g]:y0[g] + ys[g], x0[g]:x0[g] + xs[g]] = (b >> np.uint32(9)) | np.uint32(0x3f800000)  # :767
    return out


NOISE_EDGE, NOISE_CENTRE = 0.16, -3.84  # Frame.java:57-63


def noise_init(h, w, seed0, group_dim=256, colors=3, mut=None):
    """Returns (noise, A, local bits): the 5 x 5 high-pass of the local samples on mirrored coordinates (:774-787)"""
    bits = noise_local(h, w, seed0, group_dim, colors, mut)
    local = np.asarray(bits.view(F), D)
    e, c = float(f32(NOISE_EDGE)), float(f32(NOISE_CENTRE))
    box = np.stack([_windows(local[i]).sum(axis=(0, 1)) for i in range(colors)])
    return e * (box - local) + c * local, e * (box - local) + abs(c) * local, bits


NOISE_C0, NOISE_C1 = 0.00171875, 0.21828125  # Frame.java:827-828


def noise_strength(v, lut):
    """:802-825 for one of the two inputs: returns (strength before clampAsc, strength)"""
    v = np.where(v < 0, 0.0, 3.0 * v)
    i = np.where(v >= 7.0, 6, np.floor(np.minimum(v, 7.0))).astype(np.int64)
    frac = np.where(v >= 7.0, 1.0, v - i)
    s = (lut[i + 1] - lut[i]) * frac + lut[i]
    return s, np.clip(s, 0.0, 1.0)


def noise_add(planes, noise, lut, base_corr_x, base_corr_b, mut=None):
    """Returns (planes, A, (raw strength R, raw strength G))"""
    p, nz, lut = f32(planes), f32(noise), f32(lut)
    bcx, bcb = float(f32(base_corr_x)), float(f32(base_corr_b))
    c0, c1 = float(f32(NOISE_C0)), float(f32(NOISE_C1))
    if _mut(mut, "noise_corr_exchanged"):
        c0, c1 = c1, c0
    raw_r, sr = noise_strength(p[1] + p[0], lut)
    raw_g, sg = noise_strength(p[1] - p[0], lut)
    nr = sr * (c0 * nz[0] + c1 * nz[2])
    ng = sg * (c0 * nz[1] + c1 * nz[2])
    anr = sr * (c0 * np.abs(nz[0]) + c1 * np.abs(nz[2]))
    ang = sg * (c0 * np.abs(nz[1]) + c1 * np.abs(nz[2]))
    nrg, anrg = nr + ng, anr + ang
    out = np.stack([p[0] + (bcx * nrg + nr - ng), p[1] + nrg, p[2] + bcb * nrg])    # :830-832
    a = np.stack([np.abs(p[0]) + (abs(bcx) + 1.0) * anrg, np.abs(p[1]) + anrg, np.abs(p[2]) + abs(bcb) * anrg])
    return out, a, (raw_r, raw_g)


# ---- int32 arithmetic with Java's semantics ----------------------------------------------------------------------------------------
def _wrap(v):
    return ((v + 0x80000000) & 0xFFFFFFFF) - 0x80000000


def _i(v):
    return np.asarray(v).astype(np.int64)


def _add(a, b):
    return _wrap(a + b)


def _sub(a, b):
    return _wrap(a - b)


def _mul(a, b):
    return _wrap(a * b)


def _tdiv(a, n):
    """Java's a / n for n > 0: truncation toward zero"""
    return np.where(a >= 0, a // n, -((-a) // n))


def modular_to_float(a, b, scale):
    """Frame.java:437-448: the int sum wraps (:441), the conversion comes before the product. Returns (out, A)"""
    v = _i(a) if b is None else _add(_i(a), _i(b))
    out = v.astype(D) * float(f32(scale))
    return out, np.abs(out)


def tendency(a, b, c, mut=None):
    """frame/modular/ModularChannel.java:23-47 on arrays: the rising and the falling case differ in the sign of the 6 and in the
    direction of the two clamps"""
    a, b, c = _i(a), _i(b), _i(c)
    fall = (a >= b) & (b >= c)
    rise = (a <= b) & (b <= c) & ~fall
    sgn = np.where(fall, 1, -1)
    num = _add(_sub(_sub(_mul(4, a), _mul(3, c)), b), _mul(6, sgn))                 # :25, :36
    x = num // 12 if _mut(mut, "tend_div12_floor") else _tdiv(num, 12)
    d = _mul(2, _sub(a, b))
    e = _mul(2, _sub(b, c))
    odd = x & 1
    past_d = np.where(fall, _sub(x, odd) > d, _add(x, odd) < d)                     # :28, :39
    x = np.where(past_d, _add(d, sgn), x)
    odd = x & 1
    past_e = np.where(fall, _add(x, odd) > e, _sub(x, odd) < e)                     # :30, :41
    x = np.where(past_e, e, x)
    return np.where(fall | rise, x, 0)


def _unsqueeze_last_axis(avg, res, mut=None):
    """ModularChannel.java:361-387 along the last axis, all rows at once"""
    avg, res = _i(avg), _i(res)
    aw, rw = avg.shape[-1], res.shape[-1]
    assert aw in (rw, rw + 1) and avg.shape[:-1] == res.shape[:-1], "Corrupted squeeze transform"
    out = np.zeros(avg.shape[:-1] + (aw + rw,), np.int64)
    floor_half = _mut(mut, "squeeze_half_floor")
    for x in range(rw):
        a = avg[..., x]
        if x + 1 < aw:
            nxt = avg[..., x + 1]
        else:
            nxt = np.zeros_like(a) if _mut(mut, "squeeze_next_avg_zero") else a     # :372
        left = out[..., 2 * x - 1] if x > 0 else a                                  # :373
        diff = _add(res[..., x], tendency(left, a, nxt, mut))
        first = _add(a, diff >> 1 if floor_half else _tdiv(diff, 2))                # :375
        out[..., 2 * x] = first
        out[..., 2 * x + 1] = _sub(first, diff)
    if aw > rw:
        out[..., 2 * rw] = avg[..., rw]                                             # :380-384
    return out.astype(np.int32)


def inv_hsqueeze(avg, res, mut=None):
    return _unsqueeze_last_axis(avg, res, mut)


def inv_vsqueeze(avg, res, mut=None):
    """:389-413: the same recurrence down the columns"""
    return np.ascontiguousarray(_unsqueeze_last_axis(np.asarray(avg).T, np.asarray(res).T, mut).T)


RCT_PERMUTATION = ((0, 1, 2), (1, 2, 0), (2, 0, 1), (0, 2, 1), (1, 0, 2), (2, 1, 0))  # frame/modular/ModularStream.java:35-38


def rct_channels(v, rct_type, mut=None):
    """:255-326 on three equal-size channels; returns the three in their places after the permutation"""
    perm, typ = divmod(rct_type, 7)
    a, b, c = (_i(p) for p in v)
    if typ == 6:                                                                    # :309-321
        tmp = _sub(a, c >> 1)
        f = _sub(tmp, b >> 1)
        a, b, c = _add(f, b), _add(c, tmp), f
    elif typ == 5:                                                                  # :299-307
        c = _add(a, c)
        b = _add(b, _add(a, c) >> 1)
    elif typ == 4:                                                                  # :292-297
        b = _add(b, _add(a, c) >> 1)
    else:                                                                           # :267-291: bit 0 adds to the third, bit 1 to the second
        if typ & 1:
            c = _add(c, a)
        if typ & 2:
            b = _add(b, a)
    src = [p.astype(np.int32) for p in (a, b, c)]
    out = [None] * 3
    for j in range(3):
        if _mut(mut, "rct_perm_inverse"):
            out[j] = src[RCT_PERMUTATION[perm][j]]
        else:
            out[RCT_PERMUTATION[perm][j]] = src[j]                                  # :325-326
    return out


def rct(v, rct_type, mut=None):
    return np.stack(rct_channels(v, rct_type, mut))


def apply_transforms(chans, sp, rct_type=-1, rct_begin=0, mut=None):
    """the squeeze part of ModularStream.applyTransforms (:228-254), then an optional RCT (:255-326). sp: (horizontal, in place,
    begin, count) per step in forward order; undone last to first."""
    ch = [np.asarray(c, np.int32) for c in chans]
    for horizontal, in_place, begin, count in reversed(list(sp)):
        end = begin + count - 1
        offset = end + 1 if in_place else len(ch) + begin - end - 1                 # :235
        for c in range(begin, end + 1):
            ch[c] = (inv_hsqueeze if horizontal else inv_vsqueeze)(ch[c], ch[offset + c - begin], mut)
        del ch[offset:offset + count]                                               # :252-253
    if rct_type >= 0:
        ch[rct_begin:rct_begin + 3] = rct_channels(ch[rct_begin:rct_begin + 3], rct_type, mut)
    return ch
