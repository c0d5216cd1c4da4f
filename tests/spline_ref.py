"""The yardstick of the device spline stage (numpy only).

`decoder.render_splines` restates the reference (Spline.java:154-200, MathHelper.java:40-66). The one operation in which the
device may differ from it is each `(float)Math.exp(double)`: by one float neighbour, where the true value lies next to a
rounding boundary. `render_bracket` therefore draws three images from one arc table:

  mid   the operations of render_splines (asserted bit-identical to it by tests/test_splines_cpu.py), its exp pinned to the
        correctly rounded float (exp_f), so that the model gives the same bits on every CPU
  lo/hi every (float)exp result E replaced by its lower / upper float neighbour and carried through the remaining operations by
        interval arithmetic. Those are all monotone float roundings: 1 - m * E falls with E (m > 0), z < 0 flips the sign,
        factor = [erf+.lo - erf-.hi, erf+.hi - erf-.lo], (mul * f) * f takes its extremes at the interval's ends (and at 0 when
        the interval straddles it), ordered by min / max, and the running sums of lo and hi are kept apart.

The device must satisfy lo <= device <= hi at every pixel, NaN exactly where mid is NaN, and the input's bits where no arc
touches. Nothing here is tuned: there is no tolerance constant.

The `mut` argument draws deliberately wrong variants of the MODEL (tests/test_splines_cpu.py: discrimination).
Also here: `fp_exp`, the numpy restatement of jxl_fastpow.h's fp_exp with the header's coefficients, and `bin_tiles`, the
restatement of the host's tile binning (csrc/spline_host.hip)."""
import math
import os
import re

import numpy as np

from jxlatte_amd import decoder

F = np.float32
SQRT_F = F(math.sqrt(0.125))
TILE_W, TILE_H = 32, 8
HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "jxlatte_amd", "csrc", "jxl_fastpow.h")

MUTATIONS = ("sqrt_sign", "no_half", "box_short", "true_max", "per_spline_coeff", "reverse", "no_small_branch")


def _down(e):
    return np.nextafter(e, F(-np.inf), dtype=F)


def _up(e):
    return np.nextafter(e, F(np.inf), dtype=F)


def exp_f(arg):
    """(float)Math.exp(double) of a float32 array, pinned: exp in long double, rounded ONCE to float -- the correctly rounded
    float (a 64-bit significand leaves a tie-breaking doubt on ~2^-40 of the arguments), whatever SIMD exp numpy's float64
    loop uses on a given CPU. decoder.render_splines takes numpy's float64 exp; the two floats differ only where the double
    lands within its own error of a float rounding boundary (~2^-29 of the samples), and mid == render_splines is asserted on
    the model frames (tests/test_splines_cpu.py)"""
    with np.errstate(all="ignore"):
        return np.exp(arg.astype(np.longdouble)).astype(F)


def _erf3(z, args, mut):
    """MathHelper.erf of the float32 array z as (lo, mid, hi); the exp arguments (float32) are appended to `args`"""
    az = np.abs(z)
    t = (F(1) / (az * F(0.5) + F(1))).astype(F)
    u = t * F(0.17087277) - F(0.82215223)
    for cst, sign in ((1.48851587, 1), (1.13520398, -1), (0.27886807, 1), (0.18628806, -1), (0.09678418, 1), (0.37409196, 1),
                      (1.00002368, 1)):
        u = (t * u + F(cst)).astype(F) if sign > 0 else (t * u - F(cst)).astype(F)
    u = (t * u - F(1.26551223)).astype(F)
    t2 = (F(1) / (az * F(0.47047) + F(1))).astype(F)
    u2 = (t2 * ((t2 * ((t2 * F(0.7478556) - F(0.0958798)).astype(F)) + F(0.3480242)).astype(F))).astype(F)
    big = az > F(1e-4)
    if mut == "no_small_branch":
        big = np.ones_like(big)
    nzz = (-(z * z)).astype(F)
    arg = np.where(big, (nzz + u).astype(F), nzz).astype(F)
    m = np.where(big, t, u2).astype(F)
    if args is not None:
        args.append(arg.ravel().copy())
    e = exp_f(arg)
    out = []
    for ev in (_up(e), e, _down(e)):  # 1 - m * E falls with E: the upper neighbour gives the lower bound
        a = (F(1) - (m * ev).astype(F)).astype(F)
        out.append(a)
    lo, mid, hi = np.minimum(out[0], out[2]), out[1], np.maximum(out[0], out[2])
    neg = z < 0
    return (np.where(neg, -hi, lo).astype(F), np.where(neg, -mid, mid).astype(F), np.where(neg, -lo, hi).astype(F))


def arc_table(splines, bcx, bcb, width, height, mut=None):
    """decoder.spline_arc_table, or one of its two arc-level mutations"""
    if mut == "per_spline_coeff":  # every spline with its own coefficients (what the reference's dropped id would select)
        out = []
        for sp in splines:
            out += decoder.spline_arc_table([sp], bcx, bcb, width, height)
        return out
    table = decoder.spline_arc_table(splines, bcx, bcb, width, height)
    if mut == "true_max":  # MathHelper.max as a true maximum: maxDist and the box change
        out = []
        for ay, ax, sigma, inv_sigma, vals, box in table:
            mc = max(F(0.01), vals[0], vals[1], vals[2])
            with np.errstate(all="ignore"):
                md = F(np.sqrt(np.float64(F(F(F(-2) * sigma) * sigma * F(F(F(math.log(0.1)) * F(3)) - mc)))))
            if not np.isfinite(md):
                continue
            rnd = lambda v: int(np.trunc(np.clip(F(v + F(0.5)), -2**31, 2**31 - 1)))
            xb, xe = max(0, rnd(F(ax - md))), min(width - 1, rnd(F(ax + md)))
            yb, ye = max(0, rnd(F(ay - md))), min(height - 1, rnd(F(ay + md)))
            if xb <= xe and yb <= ye:
                out.append((ay, ax, sigma, inv_sigma, vals, (xb, xe, yb, ye)))
        return out
    return table


def render_bracket(planes, splines, bcx, bcb, mut=None, collect_args=False):
    """planes: (3, H, W) float32. Returns dict(lo, mid, hi: (3, H, W) float32; touched: (H, W) bool; weight: (H, W) float64, the
    sum over arcs and channels of |mul| * factor^2 ... of |term| (what the bracket's width is measured against); args: the exp
    arguments as one float32 array when collect_args; arcs: the table)"""
    planes = np.asarray(planes, F)
    _, H, W = planes.shape
    table = arc_table(splines, bcx, bcb, W, H, mut)
    if mut == "reverse":
        table = table[::-1]
    lo, mid, hi = planes.copy(), planes.copy(), planes.copy()
    touched = np.zeros((H, W), bool)
    weight = np.zeros((H, W), np.float64)
    args = [] if collect_args else None
    half = F(1.0) if mut == "no_half" else F(0.5)
    for ay, ax, sigma, inv_sigma, vals, (xb, xe, yb, ye) in table:
        if mut == "box_short":
            xe -= 1
            if xe < xb:
                continue
        ys = np.arange(yb, ye + 1, dtype=F)[:, None]
        xs = np.arange(xb, xe + 1, dtype=F)[None, :]
        dy, dx = (ys - ay).astype(F), (xs - ax).astype(F)
        dist = np.sqrt(((dy * dy).astype(F) + (dx * dx).astype(F)).astype(np.float64)).astype(F)
        sl = (slice(yb, ye + 1), slice(xb, xe + 1))
        with np.errstate(all="ignore"):
            za = (((half * dist).astype(F) + SQRT_F).astype(F) * inv_sigma).astype(F)
            zb = (((half * dist).astype(F) + (SQRT_F if mut == "sqrt_sign" else -SQRT_F)).astype(F) * inv_sigma).astype(F)
            a_lo, a_mid, a_hi = _erf3(za, args, mut)
            b_lo, b_mid, b_hi = _erf3(zb, args, mut)
            f_lo, f_mid, f_hi = (a_lo - b_hi).astype(F), (a_mid - b_mid).astype(F), (a_hi - b_lo).astype(F)
            straddle = (f_lo < 0) & (f_hi > 0)
            for c in range(3):
                mul = F(F(F(0.25) * vals[c]) * sigma)
                t_mid = ((mul * f_mid).astype(F) * f_mid).astype(F)
                p1 = ((mul * f_lo).astype(F) * f_lo).astype(F)
                p2 = ((mul * f_hi).astype(F) * f_hi).astype(F)
                p0 = np.where(straddle, ((mul * F(0)) * F(0)).astype(F), p1).astype(F)
                t_lo = np.minimum(np.minimum(p1, p2), p0)
                t_hi = np.maximum(np.maximum(p1, p2), p0)
                mid[c][sl] = (mid[c][sl] + t_mid).astype(F)
                lo[c][sl] = (lo[c][sl] + t_lo).astype(F)
                hi[c][sl] = (hi[c][sl] + t_hi).astype(F)
                weight[sl] += np.abs(np.float64(mul) * f_mid.astype(np.float64))
        touched[sl] = True
    return dict(lo=lo, mid=mid, hi=hi, touched=touched, weight=weight, arcs=table,
                args=np.concatenate(args) if args else np.zeros(0, F))


def check_device(dev, planes, br):
    """the device assertion: (violations outside the bracket, NaN mismatches, untouched pixels changed, touched samples, touched
    samples that differ from mid)"""
    dev = np.asarray(dev, F)
    nan_mid = np.isnan(br["mid"])
    nan_bad = int(np.count_nonzero(np.isnan(dev) != nan_mid))
    with np.errstate(invalid="ignore"):
        outside = ~nan_mid & ~((dev >= br["lo"]) & (dev <= br["hi"]))
    t3 = np.broadcast_to(br["touched"], dev.shape)
    untouched_bad = int(np.count_nonzero(dev.view(np.uint32)[~t3] != np.asarray(planes, F).view(np.uint32)[~t3]))
    same = (dev.view(np.uint32) == br["mid"].view(np.uint32)) | (nan_mid & np.isnan(dev))
    return int(np.count_nonzero(outside)), nan_bad, untouched_bad, int(np.count_nonzero(t3)), int(np.count_nonzero(t3 & ~same))


# ---- fp_exp (jxl_fastpow.h) restated with the header's coefficients -----------------------------------------------------------
def fp_exp_coeffs():
    src = open(HDR).read()
    body = src[src.index("double fp_exp(double x)"):src.index("TF_PQ.fromLinear (TransferFunction.java:83-87)")]
    hi, lo = (float(v) for v in re.findall(r"__builtin_fma\(x, ([0-9.e+-]+), ", body))
    first = float(re.search(r"double Q = ([0-9.e+-]+);", body).group(1))
    rest = [float(v) for v in re.findall(r"Q = __builtin_fma\(Q, rr, ([0-9.e+-]+)\);", body)]
    return hi, lo, [first] + rest


def fp_exp(x):
    """fp_exp of a float64 array. The header's two fused multiply-adds of the range reduction are carried in long double (numpy
    has no fma; the 64-bit product leaves 2^-64 |x log2 e|, far below what is measured); the series is plain multiply + add"""
    hi, lo, q = fp_exp_coeffs()
    x = np.asarray(x, np.float64)
    with np.errstate(all="ignore"):
        n = np.rint(x * hi)
        xl = x.astype(np.longdouble)
        rr = (xl * np.longdouble(hi) - n.astype(np.longdouble)).astype(np.float64)
        rr = (xl * np.longdouble(lo) + rr.astype(np.longdouble)).astype(np.float64)
        Q = np.full_like(rr, q[0])
        for c in q[1:]:
            Q = Q * rr + c
        ni = np.where(np.isnan(n), -4000, np.clip(n, -4000, 4000)).astype(np.int64)
        v = np.ldexp(Q, ni)
    v = np.where(x < -1500.0, 0.0, v)
    v = np.where(x > 1500.0, np.inf, v)
    return v


# ---- the tile lists of csrc/spline_host.hip ------------------------------------------------------------------------------------
def bin_tiles(boxes, height, width):
    """boxes: (n, 4) ints x0, x1, y0, y1 (inclusive, inside the frame), in table order. Returns (tiles, start, lst): the non-empty
    tiles (ty * tiles_x + tx) in raster order, their CSR ranges, and per tile the arcs whose box meets it, in table order"""
    tiles_x, tiles_y = -(-width // TILE_W), -(-height // TILE_H)
    per = {}
    for i, (x0, x1, y0, y1) in enumerate(np.asarray(boxes, np.int64).reshape(-1, 4)):
        for ty in range(y0 // TILE_H, y1 // TILE_H + 1):
            for tx in range(x0 // TILE_W, x1 // TILE_W + 1):
                per.setdefault(ty * tiles_x + tx, []).append(i)
    tiles = sorted(per)
    start, lst = [0], []
    for t in tiles:
        lst += per[t]
        start.append(len(lst))
    return tiles, start, lst, (tiles_x, tiles_y)


# ---- seeded spline sets ------------------------------------------------------------------------------------------------------
def random_splines(seed, n, height, width, points=(2, 6), sigma=(3, 9), color=200, margin=0, quant_adjust=0, step=None):
    """n splines of `points` control points inside the frame grown by `margin` pixels on every side; coeffSigma[0] from `sigma`
    (sigma ~ 0.33 x that), the other sigma coefficients small; colour coefficients up to +-color. step: the largest move
    between neighbouring control points (short splines)"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        k = int(rng.integers(points[0], points[1] + 1))
        if step is None:
            cp = np.stack([rng.integers(-margin, height + margin, k), rng.integers(-margin, width + margin, k)], axis=1)
        else:
            p0 = np.array([rng.integers(-margin, height + margin), rng.integers(-margin, width + margin)])
            cp = p0 + np.cumsum(rng.integers(-step, step + 1, (k, 2)), axis=0)
        coeff = np.zeros((4, 32), np.int64)
        coeff[:3, :8] = rng.integers(-color, color + 1, (3, 8))
        coeff[3, 0] = rng.integers(sigma[0], sigma[1] + 1)
        coeff[3, 1:4] = rng.integers(-1, 2, 3)
        out.append(dict(quant_adjust=quant_adjust, control=[(int(y), int(x)) for y, x in cp], coeff=coeff.tolist()))
    return out


def random_planes(seed, height, width):
    """float planes with negative values, -0.0f and exact zeros"""
    rng = np.random.default_rng(seed)
    p = rng.normal(0, 0.5, (3, height, width)).astype(F)
    r = rng.random((3, height, width))
    p[r < 0.05] = F(-0.0)
    p[r > 0.97] = F(0.0)
    return p
