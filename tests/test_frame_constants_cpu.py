"""The constants of a frame that the host now builds once per frame description (finalize_tables) where every workgroup used to
rebuild them: the EPF's inverse-sigma plane (host.hip, build_inv_sigma) and the two dequantisation tables of the persistent IDCT
launch (k_idct_wg3.hip, wg3_build_tables). Both builders are reached through hooks outside the C ABI and need no device; they are
held to the reference's expressions written in numpy float32 -- every operation one correctly rounded IEEE f32 operation, as on the
device -- and equality is on bit patterns."""
import ctypes as C

import numpy as np

from jxlatte_amd import _lib

F = np.float32


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def inv_sigma_np(hf_mul, sharp, gs, lut):
    """Frame.java:552-571: sigma = globalScale * lut[sharpness] / hfMultiplier, then its inverse"""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        sigma = F(gs) * np.asarray(lut, F)[sharp] / hf_mul.astype(F)
        return F(1) / sigma


def build_inv_sigma(hf_mul, sharp, gs, lut):
    lib = _lib.load()
    fn = lib.jxl_debug_build_inv_sigma
    fn.restype, fn.argtypes = None, [C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_void_p, C.c_void_p]
    hf = np.ascontiguousarray(hf_mul, np.int32)
    sh = np.ascontiguousarray(sharp, np.int32)
    l8 = np.ascontiguousarray(lut, np.float32)
    out = np.full(hf.shape, np.nan, np.float32)
    fn(hf.ctypes.data, sh.ctypes.data, hf.size, C.c_float(gs), l8.ctypes.data, out.ctypes.data)
    return out


def wg3_tables_np(qb, qbn, sf):
    """HFCoefficients.java:309-315 per value q = -64 .. 63 and :299 per hfMultiplier 1 .. 255 (entry 0 as 1)"""
    qb, sf, qbn = np.asarray(qb, F), np.asarray(sf, F), F(qbn)
    q = np.arange(-64, 64, dtype=np.int32)
    with np.errstate(divide="ignore", invalid="ignore"):
        gen = q.astype(F) - qbn / q.astype(F)
    qt = np.stack([np.where(q == 0, F(0), np.where(q == 1, qb[c], np.where(q == -1, -qb[c], gen))) for c in range(3)]).astype(F)
    m = np.maximum(np.arange(256, dtype=np.int32), 1).astype(F)
    st = np.stack([sf[c] / m for c in range(3)]).astype(F)
    return np.concatenate([qt.ravel(), st.ravel()])


def wg3_tables(qb, qbn, sf):
    lib = _lib.load()
    fn = lib.jxl_debug_wg3_tables
    fn.restype, fn.argtypes = None, [C.c_void_p, C.c_float, C.c_void_p, C.c_void_p]
    a, b = np.ascontiguousarray(qb, np.float32), np.ascontiguousarray(sf, np.float32)
    out = np.full(3 * 128 + 3 * 256, np.nan, np.float32)
    fn(a.ctypes.data, C.c_float(qbn), b.ctypes.data, out.ctypes.data)
    return out


def planted_maps(bh=9, bw=17, seed=5):
    """sharpness 0 (sigma 0 -> inf), multipliers 1, 255, 256, 4096 and a negative one, among random cells"""
    rng = np.random.default_rng(seed)
    sh = rng.integers(0, 8, (bh, bw)).astype(np.int32)
    hf = rng.integers(1, 16, (bh, bw)).astype(np.int32)
    sh[0, :8] = np.arange(8)
    sh[1, 0] = 0
    hf[2, :5] = [1, 255, 256, 4096, -3]
    sh[2, :5] = [7, 6, 5, 4, 3]
    hf[3, :2] = [4096, -1]
    sh[3, :2] = [0, 0]
    return hf, sh


LUT = [F(F(i) / F(7.0)) * F(0.46) if i < 7 else F(0.46) for i in range(8)]


def test_inverse_sigma_builder_matches_the_float32_formula():
    hf, sh = planted_maps()
    gs = F(65536.0) / F(2500)
    got = build_inv_sigma(hf, sh, gs, LUT)
    exp = inv_sigma_np(hf, sh, gs, LUT)
    assert np.array_equal(_bits(got), _bits(exp))
    assert np.isposinf(got[1, 0]) and np.isposinf(got[0, 0]), "sharpness 0: sigma 0, inverse +inf"
    assert got[2, 4] < 0 and np.isfinite(got[2, 4]), "a negative multiplier passes through"
    assert np.signbit(got[3, 1]) and np.isinf(got[3, 1]), "0 / negative = -0, its inverse -inf"
    assert np.isfinite(got[2, :4]).all() and (got[2, :4] > 0).all()


def test_inverse_sigma_builder_with_a_denormal_sigma():
    hf, sh = planted_maps(seed=6)
    gs = F(3e-38)  # times lut < 0.46, over multipliers up to 4096: sigma falls below the smallest normal
    exp = inv_sigma_np(hf, sh, gs, LUT)
    with np.errstate(divide="ignore", under="ignore"):
        sigma = F(gs) * np.asarray(LUT, F)[sh] / hf.astype(F)
    tiny = np.finfo(np.float32).tiny
    assert ((np.abs(sigma) < tiny) & (sigma != 0)).any(), "the case holds denormal sigmas"
    got = build_inv_sigma(hf, sh, gs, LUT)
    assert np.array_equal(_bits(got), _bits(exp))
    assert np.isinf(got[(np.abs(sigma) < F(2.0 ** -128)) & (sigma != 0)]).all(), "their inverses overflow"


def test_inverse_sigma_builder_other_lut_and_scale():
    rng = np.random.default_rng(11)
    hf, sh = planted_maps(33, 40, seed=12)
    for _ in range(4):
        lut = rng.random(8).astype(F) * F(2)
        gs = F(rng.random() * 40 + 0.01)
        assert np.array_equal(_bits(build_inv_sigma(hf, sh, gs, lut)), _bits(inv_sigma_np(hf, sh, gs, lut)))


def test_idct_tables_match_the_float32_formulas():
    from jxlatte_amd import synth
    gs = F(65536.0) / F(2500)
    cases = [(synth.DEFAULT_QUANT_BIAS, synth.DEFAULT_QBIAS_NUM, [F(gs * F(0.8)), gs, gs]),
             ([0.5, 1.25, 0.875], 0.3, [F(3.7), F(0.011), F(901.5)]),
             ([1e-40, 3e38, -0.25], 1e-39, [F(1e-38), F(3e38), F(-2.5)])]  # denormal and huge entries, a negative factor
    for qb, qbn, sf in cases:
        got = wg3_tables(qb, qbn, sf)
        exp = wg3_tables_np(qb, qbn, sf)
        assert got.shape == exp.shape == (1152,)
        assert np.array_equal(_bits(got), _bits(exp)), (qb, qbn, sf)
        q = got[:384].reshape(3, 128)
        assert (q[:, 64] == 0).all() and np.array_equal(_bits(q[:, 65]), _bits(np.asarray(qb, F)))
        assert np.array_equal(_bits(q[:, 63]), _bits(-np.asarray(qb, F)))
        s = got[384:].reshape(3, 256)
        assert np.array_equal(_bits(s[:, 0]), _bits(s[:, 1])) and np.array_equal(_bits(s[:, 1]), _bits(np.asarray(sf, F)))
