"""The CPU oracle against tests/pixel_ref64.py, the second model of the stages outside the VarDCT pixel path: the LF stage, k-times
upsampling, noise synthesis, modularToFloat and the Modular transforms. The model was written from the reference's Java in whole-array
numpy, so that a misreading shared by oracle/ and the kernels (compared bit for bit everywhere else) has something to disagree with.
tests/test_pixel_ref64_gpu.py puts the HIP kernels under the same bounds, with the oracle out of the assertion.

Integer stages (tendency, the inverse Squeeze steps, the 42 RCT types, the plans) and the noise generator's local samples: exact
equality, no exclusions. Float stages, per sample: |float32 result - model| <= K u (A + |model|), u = 2^-24, A the model's magnitude
companion. K per stage:

  stage                      how K was fixed                                                                     K   measured
  LF dequant + chroma        derived: the factor k = base + (f - 128) / colorFactor 2, Y = q sd 1, k Y 1, the    5       1.39
  from luma                  sum with q sd 1 (LFCoefficients.java:68-92); int -> float of |q| <= 2000 is exact
  LF smoothing               measured (nonlinear: the gap switches the blend, 4 sd |sample - weighted| steep):  34      16.65
                             K = 2 x the largest over LF_CASES and the frame's LF groups, rounded up
  LF stage inside a frame    LF smoothing + IDCT class 8 of tests/test_vardct_ref64_cpu.py (28): the frame's    62       5.47
                             blocks are DCT8 without HF coefficients, so a pixel is its cell's LF sample
  k-times upsampling         derived: 25 products, 24 sums, the first product passes through all of them        25       2.36
                             (Frame.java:251); the clamp (:254) rounds nothing
  noise high-pass            derived: the same count (Frame.java:782)                                           25       1.70
  noise add                  measured (nonlinear: the LUT slope times 3 amplifies the rounding of y +- x):      33      16.47
                             K = 2 x the largest over both correlation pairs, rounded up
  modularToFloat             derived: the int -> float conversion 1, the product 1 (Frame.java:441, 447)         2       0.89

"measured" is the largest |oracle - model| / (u (A + |model|)) over this file's inputs, on the CPU oracle, printed by every test
before it asserts; it is never taken from the HIP kernels. The factor two of the measured K is the margin for a GPU's differently
ordered but equally valid float32 roundings. The derived K are kept although the measured values are far below them: they are what
the arithmetic allows.

Conditions on the inputs, asserted on the model. LF: for every shape with at least 50 interior cells each smoothing regime (gap = 0.5,
0.5 < gap < 0.75, gap >= 0.75) holds at least 10 % of the interior: 32 / 24 / 44 % at 9 x 11, 40 / 19 / 41 % at 64 x 65, 39 / 20 / 41 %
at 5 x 129, the same for extraPrecision 0 (scaledDequant x 4) and extraPrecision 2 (x 8, see pixel_ref64_cases.LF_SD_MUL); the
production triple unscaled stays at 100 / 0 / 0. Upsampling: every case runs a standard normal plane (2 to 8 % of the 37 x 50 outputs
clamp), an all-negative plane, and the all-negative plane under the negated weights -- the four tiles of k = 2 are mirror images of
one another, so their weights sum to one sign, and only one of the two runs drives totals above zero, where the reference's max starts
at Float.MIN_VALUE; over the three runs of each 37 x 50 case clamped outputs make up 36 to 64 %, the rest is unclamped (both at least
10 %), and every case has outputs at Float.MIN_VALUE. Noise add:
both clamps of the strength occur, and the >= 7 branch.

The mutation table at the end shows that the checks discriminate: every deliberately wrong variant of the MODEL is told from the oracle
on every input listed for it, an integer stage by a differing sample, a float stage by missing the bound by at least 100 K."""
import numpy as np
import pytest

import pixel_ref64 as M
import pixel_ref64_cases as C
from jxlatte_amd import synth

F = np.float32
K = {"lf_dequant": 5, "lf_smooth": 34, "lf_frame": 34 + 28, "upsample": 25, "noise_conv": 25, "noise_add": 33, "to_float": 2}


def ratio(got, model, companion, what, k):
    """the K that `got` needs against the model; printed, then asserted"""
    got = np.asarray(got)
    assert np.isfinite(got).all() and np.isfinite(model).all(), what
    r = M.error_ratio(got, model, companion)
    print("%s needs K = %.2f of %d" % (what, r, k))
    assert r <= k, (what, r, k)
    return r


def same(got, exp, what):
    """integer stages: equal sample for sample (and of the same shape and type)"""
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.shape == exp.shape and got.dtype == exp.dtype == np.int32, (what, got.shape, exp.shape, got.dtype, exp.dtype)
    assert np.array_equal(got, exp), "%s: %d samples differ" % (what, int((got != exp).sum()))


def same_list(got, exp, what):
    assert len(got) == len(exp), (what, len(got), len(exp))
    for i, (a, b) in enumerate(zip(got, exp)):
        same(a, b, "%s channel %d" % (what, i))


# ---- LF stage ----------------------------------------------------------------------------------------------------------------------
def lf_regime_check(gap, shape, production=False):
    """the condition on the LF inputs (module docstring); returns the shares"""
    shares = M.lf_regimes(gap)
    print("LF %s regimes (gap = 0.5 / between / >= 0.75): %.0f %% / %.0f %% / %.0f %%" % ((shape,) + tuple(100 * s for s in shares)))
    if production:
        assert shares[0] == 1.0
    elif gap.size >= C.LF_MIN_INTERIOR:
        assert min(shares) >= C.LF_MIN_SHARE, (shape, shares)
    return shares


def lf_check(run, shape, ep, mul):
    """run(q, sd, ep, smooth) -> float32 planes: both forms of the stage against the model"""
    q, sd = C.lf_quant(shape), C.lf_sd(mul)
    x, a, gap = M.lf_stage(q, sd, ep, smooth=False, **C.LF_ARGS)
    assert gap is None
    ratio(run(q, sd, ep, False), x, a, "LF dequant %s ep %d" % (shape, ep), K["lf_dequant"])
    x, a, gap = M.lf_stage(q, sd, ep, smooth=True, **C.LF_ARGS)
    got = run(q, sd, ep, True)
    ratio(got, x, a, "LF smoothing %s ep %d x%d" % (shape, ep, mul), K["lf_smooth"])
    if min(shape) < 3:
        assert gap is None and np.array_equal(got, run(q, sd, ep, False))  # no interior: unsmoothed
    else:
        assert gap.shape == (shape[0] - 2, shape[1] - 2)
        lf_regime_check(gap, shape, production=(mul == 1))
        border = np.ones(shape, bool)
        border[1:-1, 1:-1] = False
        assert np.array_equal(got[:, border], run(q, sd, ep, False)[:, border])  # border cells are copied


@pytest.mark.parametrize("shape,ep,mul", C.LF_CASES, ids=["%dx%d-ep%d-x%d" % (s + (e, m)) for s, e, m in C.LF_CASES])
def test_lf_stage(orc, shape, ep, mul):
    lf_check(lambda q, sd, ep, smooth: orc.lf_dequant(q, sd, extra_precision=ep, adaptive_smoothing=smooth, **C.LF_ARGS), shape, ep, mul)


LF_FRAME = dict(width=2072, height=40, ep=0, mul=4, x_factor_lf=140, b_factor_lf=100)  # 5 x 259 cells: LF groups of 256 and of 3 columns


def lf_frame():
    """(frame, [integer LF image per LF group]): DCT8 blocks without HF coefficients, so every pixel of the IDCT stage is its cell's LF
    sample; each LF group is smoothed on its own (its border cells are copied)"""
    fr = synth.make_vardct_frame(LF_FRAME["width"], LF_FRAME["height"], seed=23, mix="dct8", nonzero_p=0.0)
    fr["coeff"][:] = 0
    assert len(fr["lfgroups"]) == 2 and (fr["block_types"] == 0).all()
    return fr, [C.lf_quant(np.asarray(g["dct_select"]).shape, seed=2 + i) for i, g in enumerate(fr["lfgroups"])]


def lf_frame_model(fr, lfq):
    """the model's LF planes of the whole frame, each cell repeated over its 8 x 8 pixels, and the companion"""
    p = fr["params"]
    x = np.zeros((3, p.height // 8, p.width // 8))
    a = np.zeros_like(x)
    for g, q in zip(fr["lfgroups"], lfq):
        gx, ga, gap = M.lf_stage(q, C.lf_sd(LF_FRAME["mul"]), LF_FRAME["ep"], LF_FRAME["x_factor_lf"], LF_FRAME["b_factor_lf"], True,
                                 p.base_corr_x, p.base_corr_b, p.color_factor)
        if gap.size >= C.LF_MIN_INTERIOR:
            lf_regime_check(gap, q.shape[1:])
        y0, x0 = g["lfg_y"] * 256, g["lfg_x"] * 256
        x[:, y0:y0 + q.shape[1], x0:x0 + q.shape[2]] = gx
        a[:, y0:y0 + q.shape[1], x0:x0 + q.shape[2]] = ga
    return tuple(np.repeat(np.repeat(v, 8, 1), 8, 2) for v in (x, a))


def test_lf_stage_inside_a_frame(orc):
    fr, lfq = lf_frame()
    p = fr["params"]
    for g, q in zip(fr["lfgroups"], lfq):
        lf = orc.lf_dequant(q, C.lf_sd(LF_FRAME["mul"]), extra_precision=LF_FRAME["ep"], x_factor_lf=LF_FRAME["x_factor_lf"],
                            b_factor_lf=LF_FRAME["b_factor_lf"], adaptive_smoothing=True, base_corr_x=p.base_corr_x,
                            base_corr_b=p.base_corr_b, color_factor=p.color_factor)
        gx, ga, _ = M.lf_stage(q, C.lf_sd(LF_FRAME["mul"]), LF_FRAME["ep"], LF_FRAME["x_factor_lf"], LF_FRAME["b_factor_lf"], True,
                               p.base_corr_x, p.base_corr_b, p.color_factor)
        ratio(lf, gx, ga, "LF smoothing, group %d of the frame" % g["lfg_x"], K["lf_smooth"])
        g["lf"] = [np.ascontiguousarray(lf[c]) for c in range(3)]
    ratio(orc.vardct_frame(fr, stages=1), *lf_frame_model(fr, lfq), "LF stage inside a frame", K["lf_frame"])


# ---- k-times upsampling ---------------------------------------------------------------------------------------------------------------
def up_check(run, k, shape):
    """run(plane, k, weights) -> float32 plane"""
    clamped, above = [], 0
    for name, plane, packed in C.up_runs(k, shape):
        wts = M.up_weights(k, packed)
        w32 = wts.astype(F)
        assert np.array_equal(w32, wts)  # the table holds the packed float32 values themselves
        x, a, cl = M.upsample(plane, k, wts)
        ratio(run(plane, k, w32), x, a, "upsampling k = %d %s %s" % (k, shape, name), K["upsample"])
        clamped.append(cl)
        if name != "normal":
            assert (plane < 0).all() and (x <= M.FLOAT_MIN_VALUE).all()  # nothing gets above Float.MIN_VALUE
            above += int((x == M.FLOAT_MIN_VALUE).sum())
    assert above > 0  # the quirk itself: totals above zero come out as Float.MIN_VALUE
    share = float(np.mean(clamped))
    print("upsampling k = %d %s: clamped %.1f %% (%s), %d outputs at Float.MIN_VALUE" %
          (k, shape, 100 * share, ", ".join("%.1f %%" % (100 * c.mean()) for c in clamped), above))
    if shape == (37, 50):
        assert 0.10 <= share <= 0.90, (k, share)


@pytest.mark.parametrize("k", C.UP_KS)
def test_upsampling_weights(orc, k):
    """the model's expansion of the packed coefficients (ImageHeader.java:441-470) is the oracle's table, exactly"""
    packed = np.arange(C.UP_PACKED[k], dtype=F) + F(0.5)
    assert np.array_equal(M.up_weights(k, packed).astype(F), orc.upsampling_weights(k, packed))
    packed = C.up_inputs(k, (37, 50))[0]
    assert np.array_equal(M.up_weights(k, packed).astype(F), orc.upsampling_weights(k, packed))


@pytest.mark.parametrize("shape", C.UP_SHAPES, ids=["%dx%d" % s for s in C.UP_SHAPES])
@pytest.mark.parametrize("k", C.UP_KS)
def test_upsampling(orc, k, shape):
    up_check(orc.upsample, k, shape)


# ---- noise ------------------------------------------------------------------------------------------------------------------------------
def test_noise_generator_known_answers():
    """SplitMix64's published first output for seed 0, and one batch of one generator in plain Python integers"""
    assert int(M.split_mix64(np.array([0x9e3779b97f4a7c15], np.uint64))[0]) == 0xe220a8397b1dcdaf
    mask = (1 << 64) - 1

    def sm(z):
        z = ((z ^ (z >> 30)) * 0xbf58476d1ce4e5b9) & mask
        z = ((z ^ (z >> 27)) * 0x94d049bb133111eb) & mask
        return z ^ (z >> 31)
    seed0, seed1 = 0x1234567800000009, (16 << 32) | 48
    s0, s1 = [sm((seed0 + 0x9e3779b97f4a7c15) & mask)], [sm((seed1 + 0x9e3779b97f4a7c15) & mask)]
    for i in range(7):
        s0.append(sm(s0[-1]))
        s1.append(sm(s1[-1]))
    exp = []
    for i in range(8):
        c = (s1[i] + s0[i]) & mask
        exp += [c & 0xffffffff, c >> 32]
    got = M.xorshiro_batches(seed0, np.array([seed1], np.uint64), 2)
    assert got.shape == (1, 2, 16) and got[0, 0].tolist() == exp and got[0, 1].tolist() != exp


def noise_init_check(run, h, w, gd, colors):
    """run(h, w, seed, group_dim, colors) -> float32 [colors][h][w]"""
    x, a, bits = M.noise_init(h, w, C.noise_seed(h, w), gd, colors)
    assert bits.shape == (colors, h, w) and ((bits >> 23) == 0x7f).all()  # every local sample lies in [1, 2)
    ratio(run(h, w, C.noise_seed(h, w), gd, colors), x, a, "noise high-pass %dx%d groups of %d" % (h, w, gd), K["noise_conv"])


@pytest.mark.parametrize("h,w,gd,colors", C.NOISE_INIT)
def test_noise_init(orc, h, w, gd, colors):
    noise_init_check(orc.noise_init, h, w, gd, colors)


def noise_from_exact_local_samples(h, w, gd, colors):
    """the model's local samples (exact integer arithmetic) high-passed in float32 in the reference's order (Frame.java:778-783: +=
    over iy, ix from 0f). No entry point hands out the local samples themselves, so their bit-exactness is checked through this: a
    single wrong mantissa bit of one local sample moves the output under its centre tap by 3.84 x 2^-23 or more, at least two
    spacings of float32 below 4 (no output reaches 3.84), and the comparison is bit for bit."""
    local = M.noise_local(h, w, C.noise_seed(h, w), gd, colors).view(F)
    acc = np.zeros((colors, h, w), F)
    ys, xs = M.mirror(np.arange(-2, h + 2), h), M.mirror(np.arange(-2, w + 2), w)
    for iy in range(5):
        for ix in range(5):
            tap = local[:, ys[iy:iy + h]][:, :, xs[ix:ix + w]]
            acc = acc + tap * (F(-3.84) if iy == 2 and ix == 2 else F(0.16))
            assert acc.dtype == F
    return acc


def noise_bits_check(run, h, w, gd, colors):
    got = run(h, w, C.noise_seed(h, w), gd, colors)
    exp = noise_from_exact_local_samples(h, w, gd, colors)
    assert got.dtype == F and np.array_equal(got.view(np.uint32), exp.view(np.uint32)), "%dx%d: %d samples differ" % (h, w, int((got != exp).sum()))


@pytest.mark.parametrize("h,w,gd,colors", C.NOISE_INIT)
def test_noise_local_samples_are_bit_exact(orc, h, w, gd, colors):
    noise_bits_check(orc.noise_init, h, w, gd, colors)


def noise_add_check(run, bcx, bcb):
    """run(planes, noise, lut, bcx, bcb) -> float32 planes"""
    p, nz, lut = C.noise_add_inputs()
    x, a, raw = M.noise_add(p, nz, lut, bcx, bcb)
    for r in raw:  # both clamps of the strength occur, and the >= 7 branch
        assert (r < 0).mean() > 0.02 and (r > 1).mean() > 0.02 and ((r >= 0) & (r <= 1)).mean() > 0.02
    assert (3 * (p[1] + p[0]) >= 7).mean() > 0.05 and (3 * (p[1] - p[0]) >= 7).mean() > 0.05
    ratio(run(p, nz, lut, bcx, bcb), x, a, "noise add (%g, %g)" % (bcx, bcb), K["noise_add"])


@pytest.mark.parametrize("bcx,bcb", C.NOISE_ADD_CORR)
def test_noise_add(orc, bcx, bcb):
    noise_add_check(orc.noise_add, bcx, bcb)


# ---- modularToFloat --------------------------------------------------------------------------------------------------------------------
def to_float_check(run):
    a, b = C.to_float_inputs()
    s = a.astype(np.int64) + b
    assert (np.abs(a.astype(np.int64)) > 2 ** 24).mean() > 0.9 and ((s > 2 ** 31 - 1) | (s < -2 ** 31)).mean() > 0.2  # rounds, wraps
    for scale in C.TO_FLOAT_SCALES:
        ratio(run(a, None, scale), *M.modular_to_float(a, None, scale), "modularToFloat x %g" % scale, K["to_float"])
        ratio(run(a, b, scale), *M.modular_to_float(a, b, scale), "modularToFloat of a sum x %g" % scale, K["to_float"])


def test_modular_to_float(orc):
    to_float_check(orc.modular_to_float)


# ---- integer stages -----------------------------------------------------------------------------------------------------------------------
def test_tendency_in_plain_python():
    """the array form of tendency() against ModularChannel.java:23-47 evaluated in Python integers with explicit wrapping, over every
    ordering of small and extreme operands"""
    def w(v):
        return ((v + 2 ** 31) % 2 ** 32) - 2 ** 31

    def div(a, n):
        return abs(a) // n * (1 if a >= 0 else -1)

    def one(a, b, c):
        if a >= b >= c:
            x = div(w(w(w(w(4 * a) - w(3 * c)) - b) + 6), 12)
            d, e = w(2 * w(a - b)), w(2 * w(b - c))
            if w(x - (x & 1)) > d:
                x = w(d + 1)
            if w(x + (x & 1)) > e:
                x = e
            return x
        if a <= b <= c:
            x = div(w(w(w(w(4 * a) - w(3 * c)) - b) - 6), 12)
            d, e = w(2 * w(a - b)), w(2 * w(b - c))
            if w(x + (x & 1)) < d:
                x = w(d - 1)
            if w(x - (x & 1)) < e:
                x = e
            return x
        return 0
    vals = [C.LO, C.LO + 1, -2 ** 30, -1000, -13, -7, -1, 0, 1, 5, 6, 12, 999, 2 ** 30, C.HI - 1, C.HI]
    a, b, c = (v.ravel() for v in np.meshgrid(vals, vals, vals, indexing="ij"))
    got = M.tendency(a, b, c)
    assert got.tolist() == [one(int(x), int(y), int(z)) for x, y, z in zip(a, b, c)]


def squeeze_inputs():
    """[(name, avg, res)] with the squeezed axis last"""
    out = [("random %s" % (s,), ) + C.squeeze_random(*s) for s in C.SQUEEZE_SHAPES]
    out += [("extremes %d" % i, a, r) for i, (a, r) in enumerate(C.squeeze_extremes())]
    return out + [("adversarial", ) + C.adversarial()]


def squeeze_check(hrun, vrun):
    for name, avg, res in squeeze_inputs():
        same(hrun(avg, res), M.inv_hsqueeze(avg, res), "H " + name)
        at, rt = np.ascontiguousarray(avg.T), np.ascontiguousarray(res.T)
        same(vrun(at, rt), M.inv_vsqueeze(at, rt), "V " + name)


def test_inverse_squeeze_steps(orc):
    squeeze_check(orc.inv_hsqueeze, orc.inv_vsqueeze)
    a, r = C.squeeze_random(200, 129, 129)
    assert np.array_equal(M.inv_vsqueeze(a.T, r.T), M.inv_hsqueeze(a, r).T)


@pytest.mark.parametrize("rct_type", range(42))
def test_rct(orc, rct_type):
    v = C.rct_planes(rct_type)
    same(orc.rct(v, rct_type), M.rct(v, rct_type), "rct %d" % rct_type)


def plan_inputs():
    """[(name, channels, plan)]"""
    out = [("frame %dx%dx%d" % f, ) + C.plan_frame(*f) for f in C.PLAN_FRAMES]
    return out + [("V+H %dx%d%s" % (s + (" extremes" if big else "",)), ) + C.vh_inputs(*s, big=big) for s in C.VH_SHAPES for big in (False, True)]


def rct_plan_inputs():
    """[(name, channels, plan, rctType, rctBegin)]: five channels, with and without squeeze steps in front"""
    out = []
    for t in C.RCT_BEGIN_TYPES:
        for b in (0, 1, 2):
            out.append(("rct %d at %d" % (t, b), C.rct_five_channels(), [], t, b))
            out.append(("rct %d at %d behind squeeze" % (t, b), ) + C.rct_five_channels_squeezed() + (t, b))
    return out


def test_plans(orc):
    for name, chans, sp in plan_inputs():
        same_list(orc.modular_apply(chans, sp), M.apply_transforms(chans, sp), name)
    assert any(not in_place for _, in_place, _, _ in C.plan_frame(53, 37, 3)[1])  # the residual offset of both kinds occurs
    for name, chans, sp, t, b in rct_plan_inputs():
        same_list(orc.modular_apply(chans, sp, rct_type=t, rct_begin=b), M.apply_transforms(chans, sp, t, b), name)


# ---- the checks discriminate ------------------------------------------------------------------------------------------------------------
def _lf(shape, ep, smooth=True):
    def miss(orc, mut):
        q, sd = C.lf_quant(shape), C.lf_sd(C.LF_SD_MUL[ep])
        x, a, _ = M.lf_stage(q, sd, ep, smooth=smooth, mut=mut, **C.LF_ARGS)
        got = orc.lf_dequant(q, sd, extra_precision=ep, adaptive_smoothing=smooth, **C.LF_ARGS)
        return M.error_ratio(got, x, a) / K["lf_smooth" if smooth else "lf_dequant"]
    return miss


def _up(k, run):
    def miss(orc, mut):
        _, plane, packed = C.up_runs(k, (37, 50))[run]
        wts = M.up_weights(k, packed)
        x, comp, _ = M.upsample(plane, k, wts, mut=mut)
        return M.error_ratio(orc.upsample(plane, k, wts.astype(F)), x, comp) / K["upsample"]
    return miss


def _noise_init(case):
    def miss(orc, mut):
        h, w, gd, colors = case
        x, a, _ = M.noise_init(h, w, C.noise_seed(h, w), gd, colors, mut=mut)
        return M.error_ratio(orc.noise_init(h, w, C.noise_seed(h, w), gd, colors), x, a) / K["noise_conv"]
    return miss


def _noise_add(pair):
    def miss(orc, mut):
        p, nz, lut = C.noise_add_inputs()
        x, a, _ = M.noise_add(p, nz, lut, *pair, mut=mut)
        return M.error_ratio(orc.noise_add(p, nz, lut, *pair), x, a) / K["noise_add"]
    return miss


def _int(differs):
    """an integer stage: told apart by at least one differing sample (reported as a miss of infinitely many K)"""
    return lambda orc, mut: np.inf if differs(orc, mut) else 0.0


def _squeeze(shape=None, extremes=None):
    def differs(orc, mut):
        avg, res = C.squeeze_random(*shape) if shape else C.squeeze_extremes()[extremes]
        h = not np.array_equal(orc.inv_hsqueeze(avg, res), M.inv_hsqueeze(avg, res, mut))
        at, rt = np.ascontiguousarray(avg.T), np.ascontiguousarray(res.T)
        return h and not np.array_equal(orc.inv_vsqueeze(at, rt), M.inv_vsqueeze(at, rt, mut))
    return _int(differs)


def _plan(frame):
    def differs(orc, mut):
        chans, sp = C.plan_frame(*frame)
        return any(not np.array_equal(a, b) for a, b in zip(orc.modular_apply(chans, sp), M.apply_transforms(chans, sp, mut=mut)))
    return _int(differs)


def _rct(t, begin=None):
    def differs(orc, mut):
        if begin is None:
            return not np.array_equal(orc.rct(C.rct_planes(t), t), M.rct(C.rct_planes(t), t, mut))
        chans = C.rct_five_channels()
        exp = orc.modular_apply(chans, [], rct_type=t, rct_begin=begin)
        return any(not np.array_equal(a, b) for a, b in zip(exp, M.apply_transforms(chans, [], t, begin, mut)))
    return _int(differs)


MUTATION_CASES = {
    "lf_cfl_127": [_lf((64, 65), 0, smooth=False), _lf((9, 11), 2, smooth=False), _lf((5, 129), 0)],
    "lf_gap_divided_sd": [_lf((64, 65), 2), _lf((5, 129), 2), _lf((9, 11), 2)],
    "lf_gap_per_channel": [_lf((64, 65), 0), _lf((5, 129), 2), _lf((9, 11), 0)],
    "lf_weights_exchanged": [_lf((64, 65), 0), _lf((5, 129), 2), _lf((9, 11), 0)],
    "up_max_neg_max": [_up(2, 2), _up(4, 1), _up(4, 2), _up(8, 1), _up(8, 2)],
    "up_kykx_exchanged": [_up(2, 0), _up(4, 0), _up(8, 1)],
    "noise_seed_xy_exchanged": [_noise_init(c) for c in C.NOISE_INIT[2:]],
    "noise_batch_high_low": [_noise_init(c) for c in C.NOISE_INIT[1:]],  # (not 1 x 1: the high-pass of one mirrored sample is 0)
    "noise_colour_innermost": [_noise_init(c) for c in C.NOISE_INIT[2:]],  # the cases of more than one colour
    "noise_corr_exchanged": [_noise_add(p) for p in C.NOISE_ADD_CORR],
    "rct_perm_inverse": [_rct(7 + 1), _rct(14 + 6), _rct(13, begin=1), _rct(20, begin=2)],
    "tend_div12_floor": [_squeeze((200, 129, 129)), _squeeze((7, 500, 499)), _squeeze(extremes=1), _plan((53, 37, 3))],
    "squeeze_half_floor": [_squeeze((3, 2, 1)), _squeeze((65, 33, 32)), _squeeze(extremes=2), _plan((37, 130, 4))],
    "squeeze_next_avg_zero": [_squeeze((64, 64, 64)), _squeeze((200, 129, 129)), _squeeze(extremes=0), _plan((611, 437, 3))],
}


def test_mutation_table_is_complete():
    assert set(MUTATION_CASES) == set(M.MUTATIONS) and len(M.MUTATIONS) == 14
    with pytest.raises(KeyError):
        M.rct(C.rct_planes(0), 0, mut="no such mutation")
    with pytest.raises(KeyError):
        M.lf_stage(C.lf_quant((3, 3)), C.lf_sd(4), mut="no such mutation")


@pytest.mark.parametrize("mut", M.MUTATIONS)
def test_mutation_is_detected(orc, mut):
    """a deliberately wrong MODEL is told from the oracle on EVERY input listed for it (the unmutated model passes the same inputs in
    the tests above): a float stage misses the bound by at least 100 K, an integer stage differs in at least one sample"""
    for i, miss in enumerate(MUTATION_CASES[mut]):
        assert miss(orc, None) <= 1.0, (mut, i)
        r = miss(orc, mut)
        print("%s, input %d: misses by %.3g K" % (mut, i, r))
        assert r >= 100, (mut, i, r)
