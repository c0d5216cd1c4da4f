"""An independent float64 model of the reference's spline stage (numpy only): written from SplinesBundle.java and Spline.java
alone (J/frame/features/spline), it imports nothing of jxlatte_amd and not spline_ref.py, whose bracket is built on the decoder's own
arc table. Every operation of Spline.renderSpline is done once more in float64, in the reference's order; the constants the reference
holds as floats are taken at their float values, since those are the numbers it multiplies by.

Literal quirks of the reference are the model's too: Spline(int splineID, ..) drops its id (Spline.java:23-25), so splineID stays 0
and every spline is drawn with the coefficients of spline 0 (:155); MathHelper.max(float...) keeps the SMALLER of each pair
(MathHelper.java:190-195), so maxColor is the minimum of 0.01 and the three values (:172).

render() gives three things per frame:
  x  the contribution [3][H][W], the ordered += of every arc's samples (:180-197);
  a  its magnitude companion, the sum of |0.25 * values[c] * sigma * factor^2| per sample;
  undecided  the discrete decisions that float32 and float64 may take differently, each with its distance to the tie below 1e-4 of
     the quantity's size: a box edge whose round() (MathHelper.java:36-38) lands on the other integer, an arc whose
     `arcLengthFromPrevious + arcLengthToNext >= renderDistance` (:109) differs, an `arcLength <= 0` (:160) that differs.
A case with an undecided decision is drawn again (jxl_writer_features_cases.py). The cases stay finite: no repeated control points,
no sigma that reaches 0 along a spline; render() asserts both.

The keyword arguments of render() make the WRONG expectations of test_jxl_writer_features_cpu.py."""
import math

import numpy as np

F = np.float32
SQRT_H = float(F(math.sqrt(0.5)))  # MathHelper.java:9
SQRT_F = float(F(math.sqrt(0.125)))  # :10
ADJUST = tuple(float(F(v)) for v in (0.005939697, 0.106066017, 0.098994949, 0.47135738))  # X, Y, B, sigma (Spline.java:140-143)
LOG_01_3 = float(F(F(math.log(0.1)) * F(3)))  # :173 (float)Math.log(0.1D) * 3f
TIE = 1e-4


def erf(z):
    """MathHelper.erf (MathHelper.java:40-66), the same two formulas in float64; the literals are the floats the reference holds"""
    z = np.asarray(z, np.float64)
    az = np.abs(z)
    c = [float(F(v)) for v in (0.17087277, 0.82215223, 1.48851587, 1.13520398, 0.27886807, 0.18628806, 0.09678418, 0.37409196,
                               1.00002368, 1.26551223)]
    t = 1.0 / (az * 0.5 + 1.0)  # :50
    u = t * (t * (t * (t * (t * (t * (t * (t * (t * c[0] - c[1]) + c[2]) - c[3]) + c[4]) - c[5]) + c[6]) + c[7]) + c[8]) - c[9]  # :51-52
    big = 1.0 - t * np.exp(-z * z + u)  # :53
    t2 = 1.0 / (az * float(F(0.47047)) + 1.0)  # :59
    u2 = t2 * (t2 * (t2 * float(F(0.7478556)) - float(F(0.0958798))) + float(F(0.3480242)))  # :60
    small = 1.0 - u2 * np.exp(-z * z)  # :61
    out = np.where(az > float(F(1e-4)), big, small)  # :45
    return np.where(z < 0, -out, out)  # :63-65


def compute_coeffs(coeff, quant_adjust, base_x, base_b, other_branch=False):
    """Spline.computeCoeffs (Spline.java:133-152) -> (X, Y, B, sigma), each 32 float64"""
    qa = quant_adjust / 8.0  # :138
    pos = qa >= 0
    if other_branch:
        pos = not pos
    inv_qa = 1.0 / (1.0 + qa) if pos else 1.0 - qa  # :139
    cx, cy, cb, cs = (np.asarray(c, np.float64) for c in coeff)
    y = cy * (ADJUST[1] * inv_qa)  # :145
    return cx * (ADJUST[0] * inv_qa) + float(base_x) * y, y, cb * (ADJUST[2] * inv_qa) + float(base_b) * y, cs * (ADJUST[3] * inv_qa)


def upsample_control_points(control):
    """Spline.upsampleControlPoints (:27-87) on [(x, y)] -> (Y[], X[]) float64"""
    pts = [(float(y), float(x)) for x, y in control]
    if len(pts) == 1:  # :28-34
        return [pts[0][0]], [pts[0][1]]
    assert all(pts[i] != pts[i + 1] for i in range(len(pts) - 1)), "a repeated control point: t[k + 1] - t[k] is 0"
    ext = [(2 * pts[0][0] - pts[1][0], 2 * pts[0][1] - pts[1][1])] + pts + \
          [(2 * pts[-1][0] - pts[-2][0], 2 * pts[-1][1] - pts[-2][1])]  # :36-43 the mirrored end points
    n = 16 * (len(ext) - 3) + 1  # :44
    uy, ux = [0.0] * n, [0.0] * n
    for i in range(len(ext) - 3):
        p = ext[i:i + 4]
        uy[i << 4], ux[i << 4] = p[1]  # :60-61
        t, d = [0.0] * 4, []
        for k in range(3):  # :63-67 the centripetal knots: |d| ** 0.5 as (dY^2 + dX^2) ** 0.25
            d.append((p[k + 1][0] - p[k][0], p[k + 1][1] - p[k][1]))
            t[k + 1] = t[k] + math.pow(d[k][0] * d[k][0] + d[k][1] * d[k][1], 0.25)
        for step in range(1, 16):
            knot = t[1] + 0.0625 * step * (t[2] - t[1])  # :69
            a = []
            for k in range(3):  # :70-74
                f = (knot - t[k]) / (t[k + 1] - t[k])
                a.append((d[k][0] * f + p[k][0], d[k][1] * f + p[k][1]))
            b = []
            for k in range(2):  # :75-79
                f = (knot - t[k]) / (t[k + 2] - t[k])
                b.append(((a[k + 1][0] - a[k][0]) * f + a[k][0], (a[k + 1][1] - a[k][1]) * f + a[k][1]))
            f = (knot - t[1]) / (t[2] - t[1])  # :80-82
            uy[i * 16 + step] = (b[1][0] - b[0][0]) * f + b[0][0]
            ux[i * 16 + step] = (b[1][1] - b[0][1]) * f + b[0][1]
    uy[-1], ux[-1] = pts[-1]  # :85-86
    return uy, ux


def intermediary_samples(uy, ux, undecided, who):
    """Spline.computeIntermediarySamples(1.0f) (:89-123) -> [(y, x, arcLength)]"""
    rd = 1.0
    cy, cx = uy[0], ux[0]
    nxt = 0
    arcs = [(cy, cx, rd)]  # :94
    while nxt < len(uy):
        py, px, acc = cy, cx, 0.0
        while True:
            if nxt >= len(uy):  # :100-103
                arcs.append((py, px, acc))
                break
            dy, dx = uy[nxt] - py, ux[nxt] - px
            to_next = math.sqrt(dy * dy + dx * dx)  # :108
            if abs(acc + to_next - rd) < TIE * rd:
                undecided.append("%s: arc %d: %.9g against the render distance" % (who, len(arcs), acc + to_next))
            if acc + to_next >= rd:  # :109
                f = (rd - acc) / to_next
                cy, cx = dy * f + py, dx * f + px
                arcs.append((cy, cx, rd))
                break
            acc += to_next
            py, px = uy[nxt], ux[nxt]
            nxt += 1
    return arcs


def fourier_ict(coeffs, t, magnitude=False):
    """Spline.fourierICT (:125-131); magnitude: the sum of the terms' absolute values instead"""
    i = np.arange(1, 32)
    terms = coeffs[1:] * np.cos(i * (math.pi / 32.0) * (t + 0.5))
    if magnitude:
        return abs(SQRT_H * coeffs[0]) + float(np.sum(np.abs(terms)))
    return SQRT_H * coeffs[0] + float(np.sum(terms))


def java_round(v):
    """MathHelper.round (MathHelper.java:36-38): (int)(d + 0.5f), a cast that truncates towards zero"""
    return int(math.trunc(v + 0.5))


def arc_table(sp, base_x, base_b, height, width, own_coeffs=False, other_branch=False, clip=True, true_max=False):
    """the arcs that draw, in the reference's order -> ([dict(y, x, sigma, values[3], box=(x0, x1, y0, y1), sigma_a, values_a[3]: the
    magnitude companions of the two sums)], undecided). height and
    width: the frame's bounds the boxes are clipped to (Spline.java:174-179) -- of the UPSAMPLED frame where it is upsampled
    (Frame.java:729-730 changes the header's bounds object)"""
    table, undecided = [], []
    splines = sp["splines"]
    for si, s in enumerate(splines):
        cX, cY, cB, cS = compute_coeffs(splines[si if own_coeffs else 0]["coeff"], sp["quant_adjust"], base_x, base_b, other_branch)  # :155
        uy, ux = upsample_control_points(s["control"])
        arcs = intermediary_samples(uy, ux, undecided, "spline %d" % si)
        arc_len = (len(arcs) - 2.0) * 1.0 + arcs[-1][2]  # :159
        if 0 < abs(arc_len) < TIE:
            undecided.append("spline %d: arcLength %.9g against 0" % (si, arc_len))
        if arc_len <= 0:  # :160
            continue
        for i, (ay, ax, alen) in enumerate(arcs):
            t = 31.0 * min(1.0, i * 1.0 / arc_len)  # :164-165
            vals = [fourier_ict(c, t) * alen for c in (cX, cY, cB)]  # :167-169
            sigma = fourier_ict(cS, t)  # :170
            assert abs(sigma) > 1e-3, "sigma reaches 0 along spline %d" % si
            max_color = max(0.01, *vals) if true_max else min(0.01, *vals)  # :172 MathHelper.max keeps the smaller
            arg = -2.0 * sigma * sigma * (LOG_01_3 - max_color)  # :173
            if arg < 0:  # (float)Math.sqrt of a negative: NaN bounds, nothing to draw. Only a wrong expectation comes here
                assert own_coeffs or other_branch or true_max, "maxDist is not finite"
                continue
            md = math.sqrt(arg)
            edges = []
            for v, lo, bound in ((ax - md, True, width), (ax + md, False, width), (ay - md, True, height), (ay + md, False, height)):
                def edge(q):
                    r = java_round(q)
                    if not clip:
                        return r
                    return max(0, r) if lo else min(bound - 1, r)  # :174-179
                # (the quantity compared is the distance of v + 0.5 to an integer, of size 1; float32 holds v itself to its own ulp)
                tol = TIE + 4.0 * float(np.spacing(F(abs(v))))
                if edge(v - tol) != edge(v + tol):
                    undecided.append("spline %d arc %d: a box edge at %.9g" % (si, i, v))
                edges.append(edge(v))
            table.append(dict(y=ay, x=ax, sigma=sigma, values=vals, box=tuple(edges), sigma_a=fourier_ict(cS, t, True),
                              values_a=[fourier_ict(c, t, True) * alen for c in (cX, cY, cB)]))
    return table, undecided


def render(sp, base_x, base_b, height, width, **wrong):
    """Frame.renderSplines: every arc of arc_table over its box (Spline.java:180-197) -> (x[3][H][W], a[3][H][W], undecided). With
    clip=False the boxes are those of an unbounded frame and what falls on this one is drawn"""
    table, undecided = arc_table(sp, base_x, base_b, height, width, **wrong)
    x = np.zeros((3, height, width), np.float64)
    a = np.zeros((3, height, width), np.float64)
    for arc in table:
        x0, x1, y0, y1 = arc["box"]
        x0, y0, x1, y1 = max(x0, 0), max(y0, 0), min(x1, width - 1), min(y1, height - 1)
        if x0 > x1 or y0 > y1:
            continue
        dy = np.arange(y0, y1 + 1, dtype=np.float64)[:, None] - arc["y"]  # :187-188
        dx = np.arange(x0, x1 + 1, dtype=np.float64)[None, :] - arc["x"]
        dist = np.sqrt(dy * dy + dx * dx)  # :189
        inv = 1.0 / arc["sigma"]  # :171
        factor = erf((0.5 * dist + SQRT_F) * inv) - erf((0.5 * dist - SQRT_F) * inv)  # :190-191
        for c in range(3):
            extra = 0.25 * arc["values"][c] * arc["sigma"] * factor * factor  # :192
            x[c, y0:y1 + 1, x0:x1 + 1] += extra  # :194
            a[c, y0:y1 + 1, x0:x1 + 1] += np.abs(extra)
    return x, a, undecided
