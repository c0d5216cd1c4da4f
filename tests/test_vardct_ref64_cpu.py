"""The CPU oracle against tests/vardct_ref64.py, the float64 model of the reference's VarDCT pixel path: a second witness that was
written from the reference's Java in matrices and whole-array numpy, so that a transcription slip shared by oracle/ and the kernels
(which are compared bit for bit everywhere else) has something to disagree with. tests/test_vardct_ref64_gpu.py puts the HIP kernels
under the same bound.

Per sample: |float32 result - model| <= K u (A + |model|), u = 2^-24, A the model's magnitude companion (the same computation on
absolute values). K per stage set and per size class (the longest transform edge in the frame):

  stage set   how K was fixed                                          class:    8    16    32    64   128   256
  IDCT        derived: dequantisation 3, chroma from luma 2, LLF        K      28    46    82   154   298   586
              2 (N/8) + 3, each pass N, one table rounding per pass  measured   3.5   3.1   3.7   3.1   3.9   3.5
  + Gaborish  derived: IDCT + 12 (nine products, eight sums, the        K      40    58    94   166   310   598
              three normalised weights)                              measured   2.2     -   2.5   2.2     -     -
  + EPF       measured (nonlinear): K = 2 x the largest over the        K     111     -   167   200     -     -
              staged / subsampled frames, iteration counts 1..3      measured  55.2     -  83.3  99.7     -     -
  + XYB       measured: K = 2 x the largest                             K       -     -    12     8     -     -
                                                                     measured     -     -   5.5   3.8     -     -
  stage entries: idct2d / fdct2d derived h + w + 2 (measured 1.1); Gaborish derived 12 (measured 1.6); EPF sigma derived 3
  (measured 0.8); EPF measured 17.9, K = 36; XYB measured 1.9, K = 4.
  ("-": no frame of that class runs that stage set; the staged frames are of the default mix, the subsampled ones all DCT8.)

"measured" is the largest |oracle - model| / (u (A + |model|)) over this file's inputs, on the CPU, printed by every test before it
asserts. The derived values hold with a wide margin (float32 sums err like a random walk, the count is the worst case), and they
are kept: they are what the arithmetic allows. No pixel is excluded: no 8 x 8 cell of any frame here has an inverse sigma within 1e-5
of the EPF's copy threshold (asserted). The mutation table at the end shows that the bounds discriminate: each deliberately wrong
variant of the MODEL misses the oracle by at least 100 K on every frame listed for it (the smallest margin: 248 K, one llfScale
entry of DCT64; every other one is beyond 3000 K)."""
import os
import re

import numpy as np
import pytest

import vardct_ref64 as M
import vardct_ref64_cases as C
from jxlatte_amd import abi

F = np.float32
IDCT, GAB, EPF, XYB = 1, 3, 7, 15  # stage sets: abi.STAGE_IDCT | STAGE_GAB | STAGE_EPF | STAGE_XYB, float32 planes out


def k_idct(n):
    """roundings on the longest path of one sample of an n-point block: dequantisation 3 (HFCoefficients.java:310-314), chroma from
    luma 2 (:187), LLF two passes of n/8 terms, two scalings and llfScale (:218-225), the column pass and the row pass n each
    (MathHelper.java:72-77) and the float rounding of one table entry per pass (:26)"""
    return 3 + 2 + (2 * (n // 8) + 3) + 2 * n + 2


K = {IDCT: {n: k_idct(n) for n in (8, 16, 32, 64, 128, 256)},
     GAB: {n: k_idct(n) + 12 for n in (8, 16, 32, 64, 128, 256)},
     EPF: {8: 111, 32: 167, 64: 200},   # 2 x measured, see the table
     XYB: {32: 12, 64: 8}}
K_STAGE = {"idct2d": lambda h, w: h + w + 2, "gab": 12, "epf_sigma": 3, "epf": 36, "xyb": 4}  # EPF, XYB: 2 x measured
MAX_EXCLUDED = 0.001


def check(got, frame, stages, what):
    """got (float32 planes of `stages`) against the model under K[stages][size class]; returns the ratio it needed"""
    x, a, undecided = M.decode(frame, stages)
    assert undecided.mean() <= MAX_EXCLUDED
    r = M.error_ratio(got, x, a, np.broadcast_to(undecided, x.shape))
    k = K[stages][C.size_class(frame)]
    print("%s: stages %d class %d needs K = %.2f of %d, %d samples excluded" % (what, stages, C.size_class(frame), r, k, int(undecided.sum()) * 3))
    assert r <= k, (what, stages, r, k)
    return r


# ---- facts about the format, exact in float64 ----------------------------------------------------------------------------------
def test_type_table_equals_abi():
    assert len(M.TYPES) == len(abi.TRANSFORM_TYPES) == 27
    for t in range(27):
        name, typ, par, order, meth, ph, pw = abi.TRANSFORM_TYPES[t]
        assert M.TYPES[t] == (name, typ, par, order, meth, ph, pw) and typ == t
        assert M.pixel_size(t) == abi.tt_pixel_size(t) and M.param_index(t) == abi.tt_param_index(t)
        assert M.matrix_size(t) == abi.tt_matrix_size(par)


def test_tables_equal_the_reference_source_text():
    """the 256 AFV numbers of include/jxl_tables.h (the one table the model cannot derive) and the 32 LLF scales against the literals of
    the reference's Java source, as float values; the LLF closed form of the model against both"""
    assert np.array_equal(M.LLF_SCALE, M._LLF_SCALE_TABLE)
    ref = "/root/reference/java/com/traneptora/jxlatte"
    if not os.path.isdir(ref):
        pytest.skip("reference checkout absent")
    src = open(os.path.join(ref, "frame", "group", "PassGroup.java")).read()
    body = src[src.index("AFV_BASIS ="):]
    body = body[:body.index("};")]
    vals = np.array([float(v) for v in re.findall(r"(-?\d+\.\d+(?:[eE]-?\d+)?)f", body)], np.float64)
    assert vals.size == 256
    assert np.array_equal(vals.astype(F), M.AFV_BASIS.reshape(-1).astype(F))
    src = open(os.path.join(ref, "frame", "vardct", "LLFScale.java")).read()
    vals = np.array([float(v) for v in re.findall(r"(\d\.\d+)f", src[src.index("SCALE_F"):src.index("};")])], np.float64)
    assert vals.size == 32 and np.array_equal(vals.astype(F), M.LLF_SCALE.astype(F))


def test_structure_of_the_synthesis_matrices():
    """S^T S = N I for the METHOD_DCT types; the DCT8_4 matrix is the DCT4_8 matrix with the pixel axes swapped; column 0 (the LF
    sample) of every special type is constant 1. NOT asserted, because the reference does not satisfy it: AFV1/2/3 as whole mirror images
    of AFV0. PassGroup.invertAFV mirrors the samples of the 4 x 4 AFV corner only (PassGroup.java:112-117); the 4 x 4 DCT quadrant and
    the 4 x 8 half move to the other side unmirrored (:128-146). What holds, and is asserted: the corner is the mirror image, the other
    two parts are translated."""
    for n in (1, 2, 4, 8, 16, 32, 64, 128, 256):
        s = M.synthesis(n)
        assert np.abs(s.T @ s - n * np.eye(n)).max() < 1e-12 * n
        assert np.abs(M.analysis(n) @ s - np.eye(n)).max() < 1e-12
    sp = {t: M.special_matrix(t).reshape(8, 8, 64) for t in range(27) if M.method(t) != M.METHOD_DCT}
    assert len(sp) == 9
    for t, s in sp.items():
        assert np.abs(s[:, :, 0] - 1.0).max() < 1e-12, M.NAME[t]
        assert np.linalg.matrix_rank(s.reshape(64, 64)) == 64, M.NAME[t]
    assert np.abs(sp[13] - sp[12].transpose(1, 0, 2)).max() < 1e-12
    a0 = sp[14]
    for t, (fy, fx) in ((15, (0, 1)), (16, (1, 0)), (17, (1, 1))):
        a = sp[t]
        cy, cx = slice(4 * fy, 4 * fy + 4), slice(4 * fx, 4 * fx + 4)
        corner = a0[:4, :4][::-1 if fy else 1, ::-1 if fx else 1]
        assert np.abs(a[cy, cx] - corner).max() < 1e-12
        ox = slice(0, 4) if fx else slice(4, 8)
        assert np.abs(a[cy, ox] - a0[:4, 4:]).max() < 1e-12
        assert np.abs(a[slice(0, 4) if fy else slice(4, 8), :] - a0[4:, :]).max() < 1e-12
        assert np.abs(a - a0[::-1 if fy else 1, ::-1 if fx else 1]).max() > 0.1  # the whole-block mirror does not hold


# ---- frames ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", range(27))
def test_single_type_frame(orc, t):
    """random asymmetric weights, hfMultiplier in {1, ..., 255, 256, 300, 4097} per block, |q| in {0, 1, 2, >= 64} of both signs, a
    non-constant LF field, chroma-from-luma factors that differ in every tile"""
    fr = C.type_frame(t)
    assert (fr["block_types"] == t).mean() > 0.2 and C.size_class(fr) == max(abi.tt_pixel_size(t))
    q = fr["coeff"]
    assert all((q == v).any() for v in (0, 1, -1, 2, -2, 64, -64, -777))
    muls = set(np.unique(fr["hf_mul"]).tolist())
    assert muls & {1, 2, 3, 7} and muls & {255, 256} and muls & {300, 4097} if len(fr["block_types"]) >= 16 else muls
    g = fr["lfgroups"][0]
    assert len(set(np.asarray(g["x_from_y"]).ravel().tolist())) == np.asarray(g["x_from_y"]).size > 1
    assert np.ptp(g["lf"][1]) > 0
    for p in range(17):
        for c in range(3):
            mh, mw = abi.tt_matrix_size(p)
            if mh == mw:
                w = fr["weights"][fr["woffs"][p * 3 + c]:][:mh * mw].reshape(mh, mw)
                assert not np.array_equal(w, w.T)
    check(orc.vardct_frame(fr, stages=IDCT), fr, IDCT, abi.TT_NAME[t])


@pytest.mark.parametrize("case", C.MIXED, ids=[m[0] for m in C.MIXED])
def test_mixed_frame(orc, case):
    name, w, h, seed, mix, aligned = case
    fr = C.frame(w, h, seed, mix, aligned)
    if not aligned and w >= 128:
        kx, _ = M.cfl_factor_maps(M.frame_inputs(fr))
        inp = M.frame_inputs(fr)
        straddle = sum(1 for by, bx, t in inp["blocks"] if (by * 8) // 64 != (by * 8 + M.pixel_size(t)[0] - 1) // 64
                       or (bx * 8) // 64 != (bx * 8 + M.pixel_size(t)[1] - 1) // 64)
        assert straddle > 0, "no block straddles a chroma-from-luma tile"
    check(orc.vardct_frame(fr, stages=IDCT), fr, IDCT, name)


def test_unvisited_tile_origin_reads_the_empty_cache(orc):
    """a block that straddles tiles and is visited BEFORE the block that holds the next tile's origin reads factor 0 there, not the
    tile's factor and not the base correlation (HFCoefficients.java:155-156, 183-184): the model's visiting-order rule, on a frame
    where it matters, against the oracle"""
    fr = C.frame(512, 512, 5, "all", False)
    inp = M.frame_inputs(fr)
    kx, kb = M.cfl_factor_maps(inp)
    unseen = (kb == 0.0)  # base_corr_b = 1 and |b_from_y / 84| < 1: a visited tile never has factor 0
    assert inp["p"]["base_corr_b"] == 1.0 and unseen.sum() > 0
    print("pixels that read the empty cache: %d" % int(unseen.sum()))
    check(orc.vardct_frame(fr, stages=IDCT), fr, IDCT, "empty cache")


@pytest.mark.parametrize("mode", sorted(C.SUBSAMPLINGS))
def test_subsampled_frame(orc, mode):
    """chroma from luma skipped, each channel on its own grid, Frame.invertSubsampling, then Gaborish and the EPF on full planes"""
    fr = C.subsampled_frame(mode)
    outs = {}
    for stages in (IDCT, GAB, EPF):
        outs[stages] = orc.vardct_frame(fr, stages=stages)
        check(outs[stages], fr, stages, "subsampled %s" % mode)
    assert (outs[EPF] != outs[GAB]).any(axis=0).mean() > 0.05


@pytest.mark.parametrize("name", [s[0] for s in C.STAGED])
def test_staged_frame(orc, name):
    """IDCT, + Gaborish, + EPF, + XYB; EPF iterations 0..3, Gaborish on and off, intensity target 255 and 10000; the sigma map comes
    from hf_mul and sharpness (every sharpness 0..7 present), so copied and filtered cells both occur"""
    fr = C.staged_frame(name)
    inp = M.frame_inputs(fr)
    assert set(np.unique(inp["sharpness"]).tolist()) == set(range(8))
    sig = M.epf_sigma(inp["hf_mul"], inp["sharpness"], inp["p"]["global_scale_f"], inp["p"]["epf_sharp_lut"])
    copied = sig > M.COPY_THRESHOLD
    assert 0.05 < copied.mean() < 0.95 and not M.epf_undecided_cells(sig).any()
    outs = {}
    for stages in (IDCT, GAB, EPF, XYB):
        outs[stages] = orc.vardct_frame(fr, stages=stages)
        check(outs[stages], fr, stages, name)
    if inp["p"]["epf_iters"] > 0:
        changed = (outs[EPF] != outs[GAB]).any(axis=0)
        assert changed.mean() > 0.05, "the EPF leaves the frame alone: the inputs are too wild for its weights"


# ---- the stage entry points' inputs (the GPU file runs the same ones through jxl_stage_*) ----------------------------------------
def stage_ratio(got, model, companion, what, k):
    got = np.asarray(got)
    assert np.array_equal(np.isnan(got), np.isnan(model)) and np.array_equal(np.isinf(got), np.isinf(model)), what
    fin = np.isfinite(model)
    r = M.error_ratio(got[fin], model[fin], companion[fin])
    print("%s needs K = %.2f of %d" % (what, r, k))
    assert r <= k, (what, r, k)
    return r


@pytest.mark.parametrize("h,w,t", C.IDCT2D_SIZES)
def test_stage_idct2d_fdct2d(orc, h, w, t):
    x = np.random.default_rng(h * 7 + w).standard_normal((h, w)).astype(F)
    stage_ratio(orc.idct2d(x, t), *M.idct2d(x, t), "idct2d %dx%d" % (h, w), K_STAGE["idct2d"](h, w))
    stage_ratio(orc.fdct2d(x), *M.fdct2d(x), "fdct2d %dx%d" % (h, w), K_STAGE["idct2d"](h, w))


@pytest.mark.parametrize("h,w", C.STAGE_SIZES)
def test_stage_gab_epf(orc, h, w):
    p, sig = C.stage_planes(h, w), C.stage_sigma(h, w)
    stage_ratio(orc.gab(p, *C.GAB_W), *M.gab(p, np.abs(p), *C.GAB_W), "gab %dx%d" % (h, w), K_STAGE["gab"])
    for iters in range(4):
        exp = orc.epf(p, iters, sig, 0.0, *C.EPF_ARGS)
        x, a = M.epf(p, np.abs(p), iters, sig, *C.EPF_ARGS)
        assert not M.epf_undecided_cells(sig).any()
        stage_ratio(exp, x, a, "epf %dx%d it%d" % (h, w, iters), K_STAGE["epf"])
        dead = np.repeat(np.repeat(~(sig <= M.COPY_THRESHOLD), 8, 0), 8, 1)[:h, :w]  # inf, NaN, 3.4: copied, as a class
        assert np.array_equal(exp[:, dead], p[:, dead]) and np.array_equal(x[:, dead], p[:, dead].astype(np.float64))
        if iters and h * w > 64:
            assert (exp != p).mean() > 0.1


def test_stage_epf_sigma_and_xyb(orc):
    rng = np.random.default_rng(8)
    hf = rng.integers(1, 20, size=(9, 13)).astype(np.int32)
    sh = rng.integers(0, 8, size=(9, 13)).astype(np.int32)
    par = M.params_dict(C.synth.default_params(8, 8))
    model = M.epf_sigma(hf, sh, 26.2144, par["epf_sharp_lut"])
    assert np.isinf(model).any()
    stage_ratio(orc.epf_sigma(hf, sh, 26.2144, par["epf_sharp_lut"]), model, np.abs(model), "epf sigma", K_STAGE["epf_sigma"])
    x = C.stage_planes(37, 91) * F(3.0)
    for it in (255.0, 10000.0):
        exp = orc.xyb(x, par["opsin_matrix"], par["opsin_bias"], par["cbrt_opsin_bias"], it)
        stage_ratio(exp, *M.xyb(x, np.abs(x), par["opsin_matrix"], par["opsin_bias"], par["cbrt_opsin_bias"], it), "xyb %g" % it,
                    K_STAGE["xyb"])


# ---- the tolerance discriminates ---------------------------------------------------------------------------------------------------
def _tf(name):
    return lambda: C.type_frame(abi.TT_BY_NAME[name])


def _mixed(name):
    return lambda: C.frame(*[m for m in C.MIXED if m[0] == name][0][1:])


MUTATION_CASES = {
    "no_weight_flip": [(_tf("DCT8"), IDCT), (_tf("DCT16"), IDCT), (_tf("DCT64"), IDCT)],
    "afv_flip_swapped": [(_tf("AFV1"), IDCT), (_tf("AFV2"), IDCT)],
    "afv_not_transposed": [(_tf("AFV0"), IDCT), (_tf("AFV3"), IDCT)],
    "dct84_48_exchanged": [(_tf("DCT8_4"), IDCT), (_tf("DCT4_8"), IDCT)],
    "hornuss_centre_00": [(_tf("HORNUSS"), IDCT)],
    "llf_scale_one": [(_tf("DCT16"), IDCT), (_tf("DCT32_8"), IDCT), (_tf("DCT64"), IDCT)],
    "cfl_origin_tile": [(_mixed("all_unaligned"), IDCT), (_mixed("default_unaligned"), IDCT)],
    "quant_bias_channel": [(_tf("DCT8"), IDCT), (_tf("DCT2"), IDCT)],
    "epf_no_border_mul": [(lambda: C.staged_frame("it1_gab1"), EPF), (lambda: C.staged_frame("it2_gab0"), EPF)],
    "epf_iter0_5tap": [(lambda: C.staged_frame("it3_gab1"), EPF), (lambda: C.staged_frame("it3_gab0"), EPF)],
    "gab_w_exchanged": [(lambda: C.staged_frame("it0_gab1"), GAB), (lambda: C.staged_frame("it2_gab1"), EPF)],
    "xyb_bias_sign": [(lambda: C.staged_frame("it0_gab1"), XYB), (lambda: C.staged_frame("it3_gab0"), XYB)],
}


def test_mutation_table_is_complete():
    assert set(MUTATION_CASES) == set(M.MUTATIONS) and len(M.MUTATIONS) == 12
    with pytest.raises(KeyError):
        M.special_matrix(1, mut="no such mutation")


@pytest.mark.parametrize("mut", M.MUTATIONS)
def test_mutation_is_detected(orc, mut):
    """a deliberately wrong MODEL misses the oracle by at least 100 x the tolerance on EVERY frame listed for it (the unmutated model
    passes the same frames in the tests above)"""
    for make, stages in MUTATION_CASES[mut]:
        fr = make()
        x, a, undecided = M.decode(fr, stages, mut)
        r = M.error_ratio(orc.vardct_frame(fr, stages=stages), x, a, np.broadcast_to(undecided, x.shape))
        k = K[stages][C.size_class(fr)]
        print("%s: stages %d class %d: misses by %.3g = %.3g K" % (mut, stages, C.size_class(fr), r, r / k))
        assert r >= 100 * k, (mut, stages, r, k)
