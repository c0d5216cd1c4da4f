"""The EPF tails of the fused restoration kernel after their diet -- a pixel's three quotients by one refined reciprocal behind a
window test (restore_fused_body.h, epf_quot3.h) -- held bit for bit to the oracle AND to the stage-kernel chain of the same context
(k_restore.hip keeps the plain divisions: the independent route).

Planes reach the frame path's own launch through host.restoreFused. Seeded noise at the scale of XYB samples, planted with what the
window test must send to the plain divisions: exact zeros of both signs in all three channels, a block of denormals, a block of
+-1e30; the cell maps mix cells on both sides of the skip rule in a checkerboard finer than a patch row, so patches span both. Sizes:
72x40 all edge tiles, 136x72 a 3x3 grid whose centre tile is interior, 264x112 ragged last tiles and a tile count that is no multiple
of 8, 264x136 the same for the split three-iteration pair. jxl_debug_last_restore_launches must name the promised instantiation:
| 512 (the form that keeps the plain divisions) exactly when a factor of the weights is negative.

Cell-tiled input, a quantising sink and the batch launch exist on the frame path only (the IDCT writes their input), so those cases
run synthetic frames through the runner of tests/restore_variants.py, against the oracle's decode of the same frame.
"""
import numpy as np
import pytest

import restore_variants as rv
from conftest import assert_bits_equal
from jxlatte_amd import host, synth

pytestmark = pytest.mark.gpu

SIZES = [(72, 40), (136, 72), (264, 112), (264, 136)]
PLAIN_BIT = 512


def _case(w, h, huge=True):
    rng = np.random.default_rng(9100 + 3 * w + h)
    amp = np.array([0.004, 0.05, 0.03], np.float32)[:, None, None]
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    base = np.stack([np.sin(x / 19 + c) * np.cos(y / 13 - c) for c in range(3)])
    planes = (amp * (base + 0.2 * rng.standard_normal((3, h, w)))).astype(np.float32)
    planes[:, 9:14, 20:31] = 0.0                      # exact zeros, all three channels: zero numerators
    planes[:, 14:17, 20:31] = -0.0
    planes[:, 22:27, 40:52] = np.float32(3e-41) * rng.integers(-9, 10, (3, 5, 12)).astype(np.float32)   # denormals
    big = np.where(rng.random((3, 6, 12)) < 0.5, np.float32(1e30), np.float32(-1e30))
    if huge:
        planes[:, 30:36, 8:20] = big
    planes[1, h - 3:, w - 9:] = 0.0                   # and at the frame's corner, where the mirror fix-up feeds the taps
    bh, bw = (h + 7) // 8, (w + 7) // 8
    cy, cx = np.mgrid[0:bh, 0:bw]
    # (sharpness 7, hf_mul 1) is filtered at the default header; (sharpness 0 ...) and large hf_mul fall under the skip rule
    sh = np.where((cy + cx) % 2 == 0, rng.integers(4, 8, (bh, bw)), rng.integers(0, 3, (bh, bw))).astype(np.int32)
    hf = np.where((cy + cx) % 2 == 0, rng.integers(1, 4, (bh, bw)), rng.integers(1, 16, (bh, bw))).astype(np.int32)
    return planes, hf, sh


def _params(w, h, iters, gab, **fields):
    p = synth.default_params((w + 7) // 8 * 8, (h + 7) // 8 * 8, epf_iters=iters, gab=gab)
    for k, v in fields.items():
        if isinstance(v, (list, tuple)):
            for i, e in enumerate(v):
                getattr(p, k)[i] = e
        else:
            setattr(p, k, v)
    return p


def _oracle(orc, planes, hf, sh, p):
    x = planes
    if p.gab:
        x = orc.gab(x, list(p.gab_w1), list(p.gab_w2))
    if p.epf_iters:
        sig = orc.epf_sigma(hf, sh, p.global_scale_f, list(p.epf_sharp_lut))
        x = orc.epf(x, p.epf_iters, sig, 0.0, list(p.epf_channel_scale), p.epf_pass0_sigma_scale, p.epf_pass2_sigma_scale,
                    p.epf_border_sad_mul)
    return orc.xyb(x, list(p.opsin_matrix), list(p.opsin_bias), list(p.cbrt_opsin_bias), p.intensity_target)


def _stage_chain(ctx, planes, hf, sh, p):
    x = planes
    if p.gab:
        x = host.performGabConvolution(ctx, x, list(p.gab_w1), list(p.gab_w2))
    if p.epf_iters:
        sig = host.epfInverseSigma(ctx, hf, sh, p.global_scale_f, list(p.epf_sharp_lut))
        x = host.performEdgePreservingFilter(ctx, x, p.epf_iters, sig, 0.0, list(p.epf_channel_scale), p.epf_pass0_sigma_scale,
                                             p.epf_pass2_sigma_scale, p.epf_border_sad_mul)
    m = host.OpsinInverseMatrix(list(p.opsin_matrix), list(p.opsin_bias), list(p.cbrt_opsin_bias))
    return m.invertXYB(ctx, x, p.intensity_target)


def _promised(gab, iters, plain):
    bit = PLAIN_BIT if plain and iters else 0
    if iters == 3:  # the split pair: Gaborish + the 13-tap iteration, then two iterations without Gaborish
        return [rv.code("SK_PLAIN", gab, 4) | bit, rv.code("SK_PLAIN", 0, 2) | bit]
    return [rv.code("SK_PLAIN", gab, iters) | bit]


def _check(ctx, orc, w, h, iters, gab, plain=False, huge=True, **fields):
    planes, hf, sh = _case(w, h, huge)
    p = _params(w, h, iters, gab, **fields)
    what = "restore %dx%d it%d gab%d %s" % (w, h, iters, gab, sorted(fields))
    got = host.restoreFused(ctx, planes, p, hf, sh)
    ran = host.lastRestoreLaunches(ctx)
    assert ran == _promised(gab, iters, plain), "%s: ran [%s]" % (what, "; ".join("%d = %s" % (c, rv.describe(c)) for c in ran))
    # the stage kernels of the same context: the same device arithmetic, NaN patterns included
    assert_bits_equal(got, _stage_chain(ctx, planes, hf, sh, p), what + ": against the stage kernels")
    # the oracle: +-1e30 samples overflow in the XYB stage, and an invalid operation's NaN has another sign bit on the oracle's host
    assert_bits_equal(got, _oracle(orc, planes, hf, sh, p), what + ": against the oracle", any_nan=True)


def test_the_planted_inputs_are_what_the_docstring_says(orc):
    for w, h in SIZES:
        planes, hf, sh = _case(w, h)
        p = _params(w, h, 2, True)
        s = orc.epf_sigma(hf, sh, p.global_scale_f, list(p.epf_sharp_lut))
        skip = s > np.float32(1.0 / 0.3)
        assert skip.any() and (~skip).any()
        assert (skip[:, :-1] != skip[:, 1:]).mean() > 0.25, "skip and filtered cells side by side"
        tiny = np.abs(planes[:, 22:27, 40:52])
        assert ((tiny < np.finfo(np.float32).tiny) & (tiny > 0)).any()
        assert np.signbit(planes[:, 14:17, 20:31]).all() and not np.signbit(planes[:, 9:14, 20:31]).any()
        assert (np.abs(planes[:, 30:36, 8:20]) == np.float32(1e30)).all()
    # the filter is at work outside the skipped cells
    planes, hf, sh = _case(264, 112)
    p = _params(264, 112, 2, True)
    s = orc.epf_sigma(hf, sh, p.global_scale_f, list(p.epf_sharp_lut))
    e = orc.epf(planes, 2, s, 0.0, list(p.epf_channel_scale), p.epf_pass0_sigma_scale, p.epf_pass2_sigma_scale, p.epf_border_sad_mul)
    assert (e != planes).mean() > 0.2


@pytest.mark.parametrize("gab", [True, False])
@pytest.mark.parametrize("iters", [0, 1, 2, 3])
@pytest.mark.parametrize("w,h", SIZES)
def test_planted_planes(ctx, orc, w, h, iters, gab):
    _check(ctx, orc, w, h, iters, gab)


@pytest.mark.parametrize("iters", [1, 2, 3])
@pytest.mark.parametrize("fields", [{"epf_channel_scale": (40.0, -5.0, 3.5)}, {"epf_border_sad_mul": -2.0 / 3.0}], ids=["channel_scale", "border_sad_mul"])
def test_a_negative_factor_keeps_the_unclamped_form(ctx, orc, iters, fields):
    """a negative factor makes weights above 1 and their sum unbounded: the host must choose the instantiation with the plain divisions.
    Without the +-1e30 block: that form has no window test for it to exercise, and weights above 1 carry such samples to infinity
    inside the 13-tap iteration, where the fused kernel's folded centre tap (weight exactly 1 for FINITE samples, its header) and the
    stage kernels part -- as they did before this form existed."""
    _check(ctx, orc, 264, 136, iters, True, plain=True, huge=False, **fields)


def test_a_negative_hf_mul_keeps_the_unclamped_form(ctx, orc):
    """the inverse sigma is the fourth factor: one negative hf_mul entry in the map"""
    w, h = 136, 72
    planes, hf, sh = _case(w, h, huge=False)  # (as above)
    hf[4, 8] = -3
    p = _params(w, h, 2, True)
    got = host.restoreFused(ctx, planes, p, hf, sh)
    assert host.lastRestoreLaunches(ctx) == _promised(True, 2, True)
    assert_bits_equal(got, _stage_chain(ctx, planes, hf, sh, p), "negative hf_mul: against the stage kernels")
    assert_bits_equal(got, _oracle(orc, planes, hf, sh, p), "negative hf_mul: against the oracle", any_nan=True)


# ---- the launch forms only the frame path has ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctxs():
    c = rv.Contexts()
    yield c
    c.close()


PLAIN_ROW = rv.Row("NONE", "F32", "SK_PLAIN", False)
RGB8_ROW = rv.Row("SRGB", "RGB8", "SK_SRGB_RGB8", True)
FRAME_CASES = ([rv.Case(row, "tiled", g, it, (rv.MAIN,)) for row in (PLAIN_ROW, RGB8_ROW) for g in (1, 0) for it in (1, 2)] +
               [rv.Case(RGB8_ROW, "raster", g, it, (s,)) for s in (rv.MAIN, rv.ALL_EDGE) for g in (1, 0) for it in (1, 2)] +
               [rv.Case(RGB8_ROW, "split3", 1, 3, (rv.SPLIT,))] +
               [rv.Case(row, "batch", 1, it, (rv.MAIN, rv.ALL_EDGE)) for row in (PLAIN_ROW, RGB8_ROW) for it in (1, 2)])


@pytest.mark.parametrize("case", FRAME_CASES, ids=rv.case_id)
def test_frame_path_forms(ctxs, case):
    """cell-tiled input, the sRGB / RGB8 sink and a batch of 264x112 + 72x40: against the oracle, and the hook names the instantiation"""
    problems = rv.check_case(case, ctxs, assert_bits_equal)
    assert not problems, "\n".join(problems)
