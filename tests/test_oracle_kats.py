"""CPU-only: pin the oracle with analytic known-answer tests and independent cross-checks.

The reference ships no tests or golden vectors for this path, so the oracle is
"parity unpinned" by reference fixtures; these KATs are what anchors it instead: closed-form values,
algebraic identities, an independent DCT (scipy.fft), an independent forward XYB, published PQ
points, and squeeze round trips."""
import math

import numpy as np
import pytest
import scipy.fft

from jxlatte_amd import abi, synth

F = np.float32


# ---- cosine LUT + 1-D / 2-D DCT -------------------------------------------------------------------
@pytest.mark.parametrize("l", range(0, 9))
def test_cosine_lut_closed_form(orc, l):
    s = 1 << l
    lut = orc.cosine_lut(l)
    assert lut.shape == (max(s - 1, 0), s)
    n = np.arange(1, s)[:, None].astype(np.float64)
    k = np.arange(s)[None, :].astype(np.float64)
    ref = (math.sqrt(2.0) * np.cos(math.pi * n * (k + 0.5) / s)).astype(F)
    # bit-identical: the table is nowhere near a float rounding midpoint
    assert np.array_equal(lut.view(np.uint32), ref.view(np.uint32))


def test_lut_checksum_golden(orc):
    """all 86870 entries, as one checksum committed with the tests"""
    tot = np.concatenate([orc.cosine_lut(l).ravel() for l in range(9)])
    assert tot.size == 86870
    import zlib
    assert zlib.crc32(tot.tobytes()) == GOLDEN_LUT_CRC


GOLDEN_LUT_CRC = None  # filled below at import from tests/golden/lut_crc.txt


def _load_lut_crc():
    import os
    p = os.path.join(os.path.dirname(__file__), "golden", "lut_crc.txt")
    return int(open(p).read().strip())


GOLDEN_LUT_CRC = _load_lut_crc()


@pytest.mark.parametrize("n", [1, 2, 4, 8, 16, 32, 64, 128, 256])
def test_idct1d_dc_only_is_constant(orc, n):
    x = np.zeros(n, F)
    x[0] = 3.25
    assert np.all(orc.idct1d(x) == F(3.25))


@pytest.mark.parametrize("n", [2, 4, 8, 16, 32])
def test_idct1d_single_basis_is_lut_row(orc, n):
    lut = orc.cosine_lut(int(math.log2(n)))
    for j in range(1, n):
        x = np.zeros(n, F)
        x[j] = 1.0
        assert np.array_equal(orc.idct1d(x), lut[j - 1])


@pytest.mark.parametrize("n", [2, 4, 8, 16, 32, 64, 128, 256])
def test_idct1d_against_scipy(orc, n):
    """independent implementation: out[k] = s0 + sum_n s_n sqrt2 cos(pi n (k+.5)/N) is scipy's DCT-III"""
    rng = np.random.default_rng(n)
    x = rng.standard_normal(n)
    got = orc.idct1d(x.astype(F)).astype(np.float64)
    y = x.astype(F).astype(np.float64).copy()
    y[1:] *= math.sqrt(2.0)
    ref = scipy.fft.dct(y, type=3, norm=None) / 2.0 + y[0] / 2.0  # dct3: x0 + 2 sum x_n cos(...)
    assert np.allclose(got, ref, rtol=0, atol=3e-5 * math.sqrt(n) * np.abs(x).max())


@pytest.mark.parametrize("h,w", [(8, 8), (16, 16), (32, 32), (64, 64), (128, 128), (256, 256), (16, 8), (8, 32), (64, 32), (256, 128)])
def test_idct2d_inverts_forward(orc, h, w):
    rng = np.random.default_rng(h * 1000 + w)
    x = rng.standard_normal((h, w)).astype(F)
    rt = orc.idct2d(orc.fdct2d(x))
    assert np.abs(rt - x).max() < 2e-5 * math.sqrt(h + w)


@pytest.mark.parametrize("h,w", [(4, 4), (4, 8), (8, 8), (16, 32)])
def test_idct2d_transposed_variant_is_transpose_up_to_rounding(orc, h, w):
    rng = np.random.default_rng(h + w)
    x = rng.standard_normal((h, w)).astype(F)
    a = orc.idct2d(x, transposed=False)
    b = orc.idct2d(x, transposed=True)
    assert b.shape == (w, h)
    assert np.abs(a - b.T).max() < 2e-6 * np.abs(a).max() + 1e-6


def test_fdct2d_of_constant_is_dc(orc):
    x = np.full((8, 16), 2.5, F)
    y = orc.fdct2d(x)
    assert y[0, 0] == F(2.5) and np.abs(y).sum() - abs(y[0, 0]) < 1e-5


# ---- whole VarDCT block path (dequant + LLF + transform) -------------------------------------------
def _single_type_frame(t, seed=0, **kw):
    name = abi.TT_NAME[t]
    ph, pw = abi.tt_pixel_size(t)
    return synth.make_vardct_frame(max(pw, 8) * 2, max(ph, 8) * 2, seed=seed, mix={name: 1.0}, **kw)


@pytest.mark.parametrize("t", range(27))
def test_lf_only_block_is_flat(orc, t):
    """all HF coefficients zero and a constant LF field: every transform type must reproduce the constant
    (DC-only block). quant_bias = 0 so that zero coefficients dequantise to exactly 0."""
    fr = _single_type_frame(t)
    fr["coeff"][:] = 0
    for g in fr["lfgroups"]:
        for c in range(3):
            g["lf"][c][:] = F(0.375) * (c + 1)
    p = fr["params"]
    out = orc.vardct_frame(fr, stages=abi.STAGE_IDCT)
    for c in range(3):
        assert np.abs(out[c] - F(0.375) * (c + 1)).max() < 2e-6, (abi.TT_NAME[t], c)


def test_dequant_rule_on_dct8(orc):
    """one coefficient q at (0,1) of a DCT8 block: pixel = lf + dequant(q) * sqrt2 cos(...) pattern; the weight table is made
    asymmetric, so that the transposed index of flip() (HFCoefficients.java:312-314) is told from the plain one"""
    fr = _single_type_frame(0)
    wts = np.array(fr["weights"], F, copy=True)
    wts[fr["woffs"][1]:fr["woffs"][1] + 64] *= np.linspace(0.5, 2.0, 64, dtype=F)
    fr["weights"] = wts
    fr["coeff"][:] = 0
    for g in fr["lfgroups"]:
        for c in range(3):
            g["lf"][c][:] = 0
        g["hf_mul"][:] = 2
        g["x_from_y"][:] = 0
        g["b_from_y"][:] = 0
    p = fr["params"]
    p.base_corr_x = 0.0
    p.base_corr_b = 0.0
    for q in (1, -1, 2, -7):
        fr["coeff"][:] = 0
        fr["coeff"][1, 0, 1] = q  # Y channel, block (0,0), vertical freq 0, horizontal freq 1
        out = orc.vardct_frame(fr, stages=abi.STAGE_IDCT)
        w = fr["weights"][fr["woffs"][1]:fr["woffs"][1] + 64].reshape(8, 8)
        qb, qbn = F(p.quant_bias[1]), F(p.quant_bias_numerator)
        quant = (F(q) - qbn / F(q)) if abs(q) >= 2 else (qb if q > 0 else -qb)
        sfc = F(p.scale_factor[1]) / F(2)
        assert abs(w[1, 0] - w[0, 1]) > 0.1 * abs(w[1, 0])
        co = F(F(quant * sfc) * w[1, 0])  # flip(): weight index transposed for square DCT
        lut = orc.cosine_lut(3)
        exp = np.tile((co * lut[0])[None, :], (8, 1)).astype(F)
        assert np.allclose(out[1, :8, :8], exp, rtol=1e-6, atol=1e-9), q
        assert np.all(out[1, 8:, :] == 0) and np.all(out[0] == 0) and np.all(out[2] == 0)


def test_chroma_from_luma_factor(orc):
    fr = _single_type_frame(0)
    fr["coeff"][:] = 0
    fr["coeff"][1, 3, 2] = 5
    for g in fr["lfgroups"]:
        for c in range(3):
            g["lf"][c][:] = 0
        g["x_from_y"][:] = 21
        g["b_from_y"][:] = -42
    out = orc.vardct_frame(fr, stages=abi.STAGE_IDCT)
    p = fr["params"]
    kx = F(p.base_corr_x) + F(21) / F(p.color_factor)
    kb = F(p.base_corr_b) + F(-42) / F(p.color_factor)
    y = out[1, :8, :8]
    assert np.abs(y).max() > 0
    assert np.allclose(out[0, :8, :8], kx * y, rtol=2e-6, atol=1e-9)
    assert np.allclose(out[2, :8, :8], kb * y, rtol=2e-6, atol=1e-9)


def test_afv_basis_is_orthonormal_like(orc):
    """AFV: an impulse in the first 4x4 sub-block coefficient reproduces a basis row; energy is preserved"""
    import re, os
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "jxl_tables.h")).read()
    body = hdr[hdr.index("JXL_AFV_BASIS_INIT"):hdr.index("JXL_LLF_SCALE_INIT")]
    vals = [float.fromhex(v) for v in re.findall(r"-?0x[0-9a-f.]+p[-+]\d+", body)]
    b = np.array(vals).reshape(16, 16)
    assert np.allclose(b @ b.T, np.eye(16), atol=1e-6)


# ---- Gab / EPF / XYB / transfer -----------------------------------------------------------------------
def test_gab_constant_plane_and_weights_sum(orc):
    p = np.full((3, 17, 23), 0.6, F)
    out = orc.gab(p, [0.115169525] * 3, [0.061248592] * 3)
    assert np.abs(out - F(0.6)).max() < 1e-6


def test_gab_impulse_is_kernel(orc):
    p = np.zeros((3, 9, 9), F)
    p[:, 4, 4] = 1.0
    w1, w2 = F(0.115169525), F(0.061248592)
    out = orc.gab(p, [w1] * 3, [w2] * 3)
    mult = F(1) / (F(1) + F(4) * (w1 + w2))
    assert out[0, 4, 4] == mult and out[0, 4, 5] == w1 * mult and out[0, 3, 3] == w2 * mult and out[0, 4, 6] == 0


def test_epf_sharpness_zero_is_identity(orc):
    """sharpness 0 -> sigma 0 -> invSigma = inf > 1/0.3 -> pixel copied (Frame.java:608-612)"""
    rng = np.random.default_rng(3)
    p = rng.standard_normal((3, 24, 40)).astype(F)
    lut = [0.0] + [i / 7 * 0.46 for i in range(1, 8)]
    sig = orc.epf_sigma(np.full((3, 5), 3, np.int32), np.zeros((3, 5), np.int32), 26.2144, lut)
    assert np.all(np.isinf(sig))
    for it in (1, 2, 3):
        out = orc.epf(p, it, sig, 0.0, (40.0, 5.0, 3.5), 0.9, 6.5, 2.0 / 3.0)
        assert np.array_equal(out, p)


def test_epf_constant_plane_is_fixed_point(orc):
    p = np.stack([np.full((16, 24), v, F) for v in (0.1, -0.3, 0.7)])
    sig = np.full((2, 3), 0.5, F)
    for it in (1, 2, 3):
        out = orc.epf(p, it, sig, 0.0, (40.0, 5.0, 3.5), 0.9, 6.5, 2.0 / 3.0)
        assert np.allclose(out, p, rtol=1e-6)


def test_epf_sigma_rejects_bad_sharpness(orc):
    with pytest.raises(ValueError):
        orc.epf_sigma(np.ones((1, 1), np.int32), np.full((1, 1), 8, np.int32), 1.0, [0.1] * 8)


def test_epf_smooths_towards_neighbours(orc):
    """a lone outlier with a generous sigma moves towards its neighbours, never away"""
    p = np.zeros((3, 16, 16), F)
    p[:, 8, 8] = 0.01
    sig = np.full((2, 2), 0.05, F)  # small inverse sigma = strong smoothing
    out = orc.epf(p, 1, sig, 0.0, (40.0, 5.0, 3.5), 0.9, 6.5, 2.0 / 3.0)
    assert 0 <= out[0, 8, 8] < 0.01


def test_xyb_black_and_linearity_in_matrix(orc):
    p = synth.default_params(8, 8)
    m = list(p.opsin_matrix)
    ob, cob = list(p.opsin_bias), list(p.cbrt_opsin_bias)
    z = np.zeros((3, 1, 4), F)
    out = orc.xyb(z, m, ob, cob, 255.0)
    assert np.abs(out).max() < 2e-7  # XYB (0,0,0) is black: (-cbrt(b))^3 + b
    rng = np.random.default_rng(1)
    x = (rng.standard_normal((3, 4, 4)) * 0.05).astype(F)
    a = orc.xyb(x, m, ob, cob, 255.0)
    b = orc.xyb(x, [2 * v for v in m], ob, cob, 255.0)
    assert np.array_equal(b, F(2) * a)  # doubling the matrix doubles every product exactly
    c = orc.xyb(x, m, ob, cob, 510.0)
    assert np.allclose(c, a / 2, rtol=1e-6)


def test_xyb_inverts_independent_forward_transform(orc):
    """forward XYB built independently: mix = M^-1 rgb, gamma = cbrt(mix - bias) + cbrt(bias)... in double"""
    p = synth.default_params(8, 8)
    M = np.array(list(p.opsin_matrix), np.float64).reshape(3, 3)
    bias = float(p.opsin_bias[0])
    rng = np.random.default_rng(5)
    rgb = rng.random((3, 50))
    mix = np.linalg.solve(M, rgb)
    g = np.cbrt(mix - bias) + np.cbrt(bias)
    X, Y, B = (g[0] - g[1]) / 2, (g[0] + g[1]) / 2, g[2]
    xyb = np.stack([X, Y, B]).astype(F).reshape(3, 5, 10)
    out = orc.xyb(xyb, list(p.opsin_matrix), list(p.opsin_bias), list(p.cbrt_opsin_bias), 255.0)
    assert np.allclose(out.reshape(3, 50), rgb, atol=2e-5)


def test_pq_formula_points(orc):
    """TF_PQ.fromLinear as the reference writes it (TransferFunction.java:83-87). NOTE: the reference's first
    exponent is 0.159423828125 (= 2612/16384) where SMPTE ST 2084 has m1 = 2610/16384 = 0.1593017578125; the
    oracle restates the reference, so 100 nit maps to 0.5077 instead of the standard's 0.5081."""
    x = np.array([0.0, 1.0, 0.01, 0.1, 0.37], F)
    y = orc.transfer(x, abi.TRANSFER_PQ)
    for xi, yi in zip(x.tolist(), y.tolist()):
        d = math.pow(xi, 0.159423828125)
        ref = math.pow((0.8359375 + 18.8515625 * d) / (1.0 + 18.6875 * d), 78.84375)
        assert yi == float(F(ref))
    assert y[1] == 1.0
    assert abs(y[2] - 0.5081) < 1e-3 and abs(y[3] - 0.7518) < 1e-3  # close to the published ST 2084 points


def test_srgb_points_and_quantisation(orc):
    x = np.array([0.0, 0.001, 0.0031, 0.5, 1.0], F)
    y = orc.transfer(x, abi.TRANSFER_SRGB)
    assert y[0] == 0 and y[1] == F(0.001) * F(12.92) and abs(y[3] - 0.7353569) < 1e-6 and abs(y[4] - 1.0) < 1e-6
    q = orc.transfer(np.array([-0.2, 0.0, 0.49, 0.5, 1.0, 7.0, np.nan], F), abi.TRANSFER_NONE, 255)
    assert q.tolist() == [0, 0, 125, 128, 255, 255, 0]  # (int)(v*255+0.5f), clamped; NaN -> 0 like Java


# ---- Modular -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 2), (7, 9), (16, 16), (33, 64), (64, 33), (5, 1), (1, 1), (100, 3)])
def test_squeeze_round_trip_single_steps(orc, shape):
    rng = np.random.default_rng(shape[0] * 100 + shape[1])
    img = rng.integers(-5000, 5000, size=shape).astype(np.int32)
    a, r = orc.fwd_hsqueeze(img)
    assert np.array_equal(orc.inv_hsqueeze(a, r), img)
    a, r = orc.fwd_vsqueeze(img)
    assert np.array_equal(orc.inv_vsqueeze(a, r), img)


def test_squeeze_tendency_branches_and_wraparound(orc):
    """monotone ramps exercise both clamp branches of tendency(); extreme values exercise int32 wrap"""
    ramp = np.arange(0, 64 * 37, 37, dtype=np.int32).reshape(1, 64)
    for img in (ramp, -ramp, ramp[:, ::-1].copy(), np.array([[2 ** 31 - 1, -2 ** 31, 2 ** 31 - 1, -2 ** 31, 5, 7]], np.int32)):
        a, r = orc.fwd_hsqueeze(img)
        assert np.array_equal(orc.inv_hsqueeze(a, r), img)
        a, r = orc.fwd_vsqueeze(img.T.copy())
        assert np.array_equal(orc.inv_vsqueeze(a, r), img.T)


@pytest.mark.parametrize("h,w,ch", [(37, 53, 3), (64, 64, 1), (9, 200, 4), (130, 7, 3)])
def test_full_squeeze_plan_round_trip(orc, h, w, ch):
    """forward-squeeze a random image with the default plan (test-only forward), inverse must return it"""
    rng = np.random.default_rng(h + w + ch)
    img = [rng.integers(0, 1024, size=(h, w)).astype(np.int32) for _ in range(ch)]
    sp = synth.default_squeeze_params([(h, w)] * ch)
    chans = list(img)
    for (horiz, in_place, begin, num) in sp:
        end = begin + num - 1
        offset = end + 1 if in_place else len(chans)
        for k in range(begin, end + 1):
            a, r = (orc.fwd_hsqueeze if horiz else orc.fwd_vsqueeze)(chans[k])
            chans[k] = a
            chans.insert(offset + k - begin, r)
    assert [c.shape for c in chans] == synth.squeezed_shapes([(h, w)] * ch, sp)
    out = orc.modular_apply(chans, sp)
    assert len(out) == ch and all(np.array_equal(a, b) for a, b in zip(out, img))


@pytest.mark.parametrize("rct_type", range(42))
def test_rct_inverse_of_forward(orc, rct_type):
    """forward RCT written from the spec's definitions (test-only); the oracle's inverse must undo it"""
    rng = np.random.default_rng(rct_type)
    rgb = rng.integers(0, 256, size=(3, 5, 7)).astype(np.int32)
    perm, typ = divmod(rct_type, 7)
    lut = [[0, 1, 2], [1, 2, 0], [2, 0, 1], [0, 2, 1], [1, 0, 2], [2, 1, 0]][perm]
    # the inverse ends with out[lut[j]] = v[j]  =>  before the permutation v[j] = rgb[lut[j]]
    v = [rgb[lut[j]].copy() for j in range(3)]
    a, b, c = v
    if typ == 1: c = c - a
    elif typ == 2: b = b - a
    elif typ == 3: c, b = c - a, b - a
    elif typ == 4: b = b - ((a + c) >> 1)
    elif typ == 5:
        c0 = c
        b = b - ((a + c0) >> 1)
        c = c0 - a
    elif typ == 6:
        # forward derived from the inverse (ModularStream.java:307-318): out0 = f + b, out1 = c + tmp, out2 = f
        R, G, B = a, b, c
        v1 = R - B
        tmp = B + (v1 >> 1)
        v2 = G - tmp
        v0 = tmp + (v2 >> 1)
        a, b, c = v0, v1, v2
    enc = np.stack([a, b, c]).astype(np.int32)
    out = orc.rct(enc, rct_type)
    assert np.array_equal(out, rgb)


def test_cosine_lut_is_exactly_mirror_symmetric(orc):
    """lut[n-1][N-1-k] == (-1)^n * lut[n-1][k] bit for bit, for every N: the device IDCT kernels form each product once and
    add / subtract it into the mirrored output (k_idct.hip, idct1d_reg) -- exact only because of this property"""
    for l in range(1, 9):
        lut = orc.cosine_lut(l)
        s = 1 << l
        for n in range(1, s):
            row = lut[n - 1]
            mirrored = row[::-1] * (np.float32(-1.0) if n % 2 else np.float32(1.0))
            assert np.array_equal(row.view(np.uint32), mirrored.view(np.uint32)), (s, n)
        assert not (lut == 0).any()  # no signed-zero ambiguity


def test_tendency_normalised_form(orc):
    """the r5 device form of ModularChannel.tendency (csrc/modular_tend.h: tend_n_pre / squeeze_pair_n), restated
    instruction by instruction on wrapped int32 / uint32 values: fold onto the decreasing branch with m = (b < c) ? -1 : 0,
    unsigned multiply-high division by 12, min3 / max instead of the parity clamps and the branch selects. Must equal the
    reference on the whole guarded range (|avg|, |next| < 2^23, |left| < 2^27: SqueezeRange in the same header); the guard
    is not vacuous (outside it the form does differ)."""
    def wrap(x):
        return ((x + 2**31) % 2**32) - 2**31

    def tdiv(n, d):
        return np.where(n >= 0, n // d, -((-n) // d))

    def ref(a, b, c):  # ModularChannel.java:23-47
        dec = (a >= b) & (b >= c)
        inc = (~dec) & (a <= b) & (b <= c)
        d, e = wrap(2 * wrap(a - b)), wrap(2 * wrap(b - c))
        x = tdiv(wrap(4 * a - 3 * c - b + 6), 12)
        x = np.where(wrap(x - (x & 1)) > d, wrap(d + 1), x)
        x = np.where(wrap(x + (x & 1)) > e, e, x)
        y = tdiv(wrap(4 * a - 3 * c - b - 6), 12)
        y = np.where(wrap(y + (y & 1)) < d, wrap(d - 1), y)
        y = np.where(wrap(y - (y & 1)) < e, e, y)
        return np.where(dec, x, np.where(inc, y, 0))

    def dev(a, b, c):
        bmc = wrap(b - c)
        m = bmc >> 31
        ab = wrap((bmc ^ m) - m)
        bn = wrap((b ^ m) - m)
        e2 = wrap(ab << 1)
        base = wrap(wrap(wrap(wrap(ab << 1) + ab) + 6) - wrap(bn << 2))
        k1 = wrap(1 - wrap(bn << 1))
        an = wrap((a ^ m) - m)
        n = wrap(wrap(an << 2) + base) % 2**32
        x = wrap(((n * 0xAAAAAAAB) >> 32) >> 3)
        d1 = wrap(wrap(an << 1) + k1)
        r = np.maximum(np.minimum(np.minimum(x, d1), e2), 0)
        return wrap((r ^ m) - m)
    g = np.arange(-40, 41, dtype=np.int64)
    A, B, C = np.meshgrid(g, g, g, indexing="ij")
    assert np.array_equal(ref(A, B, C), dev(A, B, C))
    rng = np.random.default_rng(5)
    for sa, sb in ((2**27, 2**23), (2**10, 2**8), (2**20, 2**23), (2**23, 2**23)):
        a = rng.integers(-sa + 1, sa, 1_000_000)
        b = rng.integers(-sb + 1, sb, a.size)
        c = rng.integers(-sb + 1, sb, a.size)
        assert np.array_equal(ref(a, b, c), dev(a, b, c)), (sa, sb)
        b2 = np.clip(a + rng.integers(-50, 51, a.size), -sb + 1, sb - 1)
        c2 = np.clip(b2 + rng.integers(-50, 51, a.size), -sb + 1, sb - 1)
        assert np.array_equal(ref(a, b2, c2), dev(a, b2, c2)), (sa, sb)
    ea = np.array([2**27 - 1, -2**27 + 1, 2**23 - 1, -2**23 + 1, 0, 1, -1, 5, -6], np.int64)
    eb = np.array([2**23 - 1, -2**23 + 1, 2**23 - 2, 0, 1, -1, 7, -9, 1000, -1000], np.int64)
    A, B, C = np.meshgrid(ea, eb, eb, indexing="ij")
    assert np.array_equal(ref(A, B, C), dev(A, B, C))
    # outputs of a guarded chunk stay guarded: |second| <= 1.07 * 2^26 < 2^27 for inputs below 2^23 and any guarded left
    a = rng.integers(-2**27 + 1, 2**27, 1_000_000)
    b = rng.integers(-2**23 + 1, 2**23, a.size)
    c = rng.integers(-2**23 + 1, 2**23, a.size)
    r = rng.integers(-2**23 + 1, 2**23, a.size)
    diff = r + ref(a, b, c)
    first = b + tdiv(diff, 2)
    assert np.abs(first - diff).max() < 2**27
    # outside the guard the short form is wrong somewhere (so the guard is what makes it exact)
    ext = np.array([2**31 - 1, -2**31, 2**30, -2**30, 2**29, 0, 1, -1], np.int64)
    A, B, C = np.meshgrid(ext, ext, ext, indexing="ij")
    assert (ref(A, B, C) != dev(A, B, C)).any()
    # and the restated reference agrees with the oracle (two-pair rows: the second pair's left is the first pair's second output)
    av = rng.integers(-1000, 1000, (2000, 2)).astype(np.int32)
    rs = rng.integers(-50, 50, (2000, 2)).astype(np.int32)
    out = orc.inv_hsqueeze(av, rs)
    t0 = ref(av[:, 0].astype(np.int64), av[:, 0].astype(np.int64), av[:, 1].astype(np.int64))
    d0 = rs[:, 0] + t0
    f0 = av[:, 0] + tdiv(d0, 2)
    t1 = ref(f0 - d0, av[:, 1].astype(np.int64), av[:, 1].astype(np.int64))
    d1 = rs[:, 1] + t1
    f1 = av[:, 1] + tdiv(d1, 2)
    assert np.array_equal(out[:, 1], f0 - d0) and np.array_equal(out[:, 2], f1) and np.array_equal(out[:, 3], f1 - d1)


def test_tendency_min_max_form(orc):
    """the device kernels' short form of ModularChannel.tendency (k_modular.hip, tend_fast_apply): min/max instead of the
    parity-and-compare clamps. Checked against the oracle's inverse squeeze through 1-pair rows (out[1] = avg + diff/2 - diff
    exposes tendency(left=avg, avg, next)) -- and directly against a numpy restatement over the safe operand range."""
    def wrap(x):
        return ((x + 2**31) % 2**32) - 2**31

    def tdiv(n, d):
        return np.where(n >= 0, n // d, -((-n) // d))

    def ref(a, b, c):
        dec = (a >= b) & (b >= c)
        inc = (~dec) & (a <= b) & (b <= c)
        d, e = wrap(2 * wrap(a - b)), wrap(2 * wrap(b - c))
        x = tdiv(wrap(4 * a - 3 * c - b + 6), 12)
        x = np.where(wrap(x - (x & 1)) > d, wrap(d + 1), x)
        x = np.where(wrap(x + (x & 1)) > e, e, x)
        y = tdiv(wrap(4 * a - 3 * c - b - 6), 12)
        y = np.where(wrap(y + (y & 1)) < d, wrap(d - 1), y)
        y = np.where(wrap(y - (y & 1)) < e, e, y)
        return np.where(dec, x, np.where(inc, y, 0))

    def fast(a, b, c):
        dec = (a >= b) & (b >= c)
        inc = (~dec) & (a <= b) & (b <= c)
        d, e = wrap(2 * wrap(a - b)), wrap(2 * wrap(b - c))
        x = tdiv(wrap(4 * a - 3 * c - b + 6), 12)
        y = tdiv(wrap(4 * a - 3 * c - b - 6), 12)
        return np.where(dec, np.minimum(np.minimum(x, wrap(d + 1)), e), np.where(inc, np.maximum(np.maximum(y, wrap(d - 1)), e), 0))
    g = np.arange(-30, 31, dtype=np.int64)
    A, B, C = np.meshgrid(g, g, g, indexing="ij")
    assert np.array_equal(ref(A, B, C), fast(A, B, C))
    rng = np.random.default_rng(11)
    for scale in (1 << 10, 1 << 20, 1 << 28):
        a = rng.integers(-scale, scale, 500_000)
        b = a + rng.integers(-scale // 4 - 1, scale // 4 + 1, a.size)
        c = b + rng.integers(-scale // 4 - 1, scale // 4 + 1, a.size)
        safe = (np.abs(a - b) < 2**29) & (np.abs(b - c) < 2**29)
        assert np.array_equal(ref(a, b, c)[safe], fast(a, b, c)[safe])
    # the device's guard (k_modular.hip tend_fast_pre / tend_fast_apply): branch masks from the SIGN of the wrapped
    # differences, `unsafe` = wrapped difference outside +-2^29 OR the subtraction overflowed. Over triples built from the
    # int32 extremes every lane is either flagged unsafe (and redone with the long form) or already equal to the reference.
    def dev_fast_and_guard(a, b, c):
        amb, bmc = wrap(a - b), wrap(b - c)
        lt, gt = amb < 0, wrap(b - a) < 0
        dec = (b >= c) & ~lt
        inc = (b <= c) & ~gt & ~dec
        d, e = wrap(2 * amb), wrap(2 * bmc)
        x = tdiv(wrap(4 * a - 3 * c - b + 6), 12)
        y = tdiv(wrap(4 * a - 3 * c - b - 6), 12)
        val = np.where(dec, np.minimum(np.minimum(x, wrap(d + 1)), e), np.where(inc, np.maximum(np.maximum(y, wrap(d - 1)), e), 0))

        def ovf(p, q, diff):  # ((p ^ q) & (p ^ diff)) < 0 on int32
            return ((p < 0) != (q < 0)) & ((p < 0) != (diff < 0))
        unsafe = (np.abs(amb) >= 2**29) | (np.abs(bmc) >= 2**29) | ovf(a, b, amb) | ovf(b, c, bmc)
        return val, unsafe
    lo, hi = -2**31, 2**31 - 1
    ext = np.array([hi, lo, hi - 1, lo + 1, hi - 2**29, lo + 2**29, 2**30, -2**30, 2**29, -2**29, 2**29 - 1, 0, 1, -1, 7, -9], np.int64)
    A, B, C = np.meshgrid(ext, ext, ext, indexing="ij")
    val, unsafe = dev_fast_and_guard(A, B, C)
    assert np.array_equal(val[~unsafe], ref(A, B, C)[~unsafe])
    assert unsafe[0, 1, 1]                      # (INT_MAX, INT_MIN, INT_MIN): a - b wraps to -1
    assert (ref(A, B, C)[unsafe] != val[unsafe]).any()  # the guard is not vacuous: the short form does differ there
    # the numpy restatement itself agrees with the oracle: row [avg, next] with residual r gives out[1] = avg + t/2... use
    # the two-pair row (avg0, avg1), residuals (0, r): second pair has left = out[1] of the first
    a = rng.integers(-1000, 1000, (2000, 2)).astype(np.int32)
    r = rng.integers(-50, 50, (2000, 2)).astype(np.int32)
    out = orc.inv_hsqueeze(a, r)
    t0 = ref(a[:, 0].astype(np.int64), a[:, 0].astype(np.int64), a[:, 1].astype(np.int64))
    diff0 = r[:, 0] + t0
    first0 = a[:, 0] + tdiv(diff0, 2)
    assert np.array_equal(out[:, 0], first0) and np.array_equal(out[:, 1], first0 - diff0)
    t1 = ref(out[:, 1].astype(np.int64), a[:, 1].astype(np.int64), a[:, 1].astype(np.int64))
    diff1 = r[:, 1] + t1
    first1 = a[:, 1] + tdiv(diff1, 2)
    assert np.array_equal(out[:, 2], first1) and np.array_equal(out[:, 3], first1 - diff1)


def test_one_colour_epf_and_gab_python_restatement(orc):
    """colors == 1 (grey, non-XYB Modular frame with restoration filters): plain-Python restatement of Frame.java:583-679 for
    one colour channel -- the distance still has three rounds, all on channel 0, each with its own channel scale (`i = colors
    == 1 ? 0 : c`) -- against the oracle's epf1 / gab1 on a small plane, every EPF iteration count"""
    F = np.float32
    rng = np.random.default_rng(12)
    h, w = 11, 13
    p = (rng.standard_normal((h, w)) * 0.05).astype(F)
    scale, pass0, pass2, bsm, inv_sigma = [F(40.0), F(5.0), F(3.5)], F(0.9), F(6.5), F(2.0) / F(3.0), F(0.8)
    step = F(1.65) * F(4) * (F(1) - F(np.sqrt(0.5)))

    def mir(c, n):
        while c < 0 or c >= n:
            c = -c - 1 if c < 0 else 2 * n - 1 - c
        return c
    cross = [(0, 0), (0, -1), (0, 1), (-1, 0), (1, 0)]
    dcross = cross + [(-1, 1), (1, 1), (1, -1), (-1, -1), (0, -2), (0, 2), (2, 0), (-2, 0)]

    def run(src, iters):
        cur = src.copy()
        for i in range(3):
            if i == 0 and iters < 3:
                continue
            if i == 2 and iters < 2:
                break
            ss = step * (pass0 if i == 0 else pass2 if i == 2 else F(1))
            taps = dcross if i == 0 else cross
            out = np.empty_like(cur)
            for y in range(h):
                for x in range(w):
                    sw, sc = F(0), F(0)
                    for (ty, tx) in taps:
                        d = F(0)
                        for c in range(3):
                            if i == 2:
                                d = F(d + F(abs(F(cur[y, x] - cur[mir(y + ty, h), mir(x + tx, w)]))) * scale[c])
                            else:
                                for (qy, qx) in cross:
                                    a = cur[mir(y + qy, h), mir(x + qx, w)]
                                    b = cur[mir(y + ty + qy, h), mir(x + tx + qx, w)]
                                    d = F(d + F(abs(F(a - b))) * scale[c])
                        if (y & 7) in (0, 7) or (x & 7) in (0, 7):
                            d = F(d * bsm)
                        v = F(F(1) - F(F(d * ss) * inv_sigma))
                        wgt = v if v > 0 else F(0)
                        sw = F(sw + wgt)
                        sc = F(sc + F(cur[mir(y + ty, h), mir(x + tx, w)] * wgt))
                    out[y, x] = F(sc / sw)
            cur = out
        return cur
    for iters in (1, 2, 3):
        got = orc.epf1(p, iters, None, float(inv_sigma), [float(s) for s in scale], float(pass0), float(pass2), float(bsm))
        exp = run(p, iters)
        assert np.array_equal(got.view(np.uint32), exp.view(np.uint32)), iters
    # Gaborish of one channel: its own weights, clamped edges (Frame.java:505-542)
    w1, w2 = F(0.115169525), F(0.061248592)
    mult = F(1) / (F(1) + F(4) * (w1 + w2))
    exp = np.empty_like(p)
    for y in range(h):
        n, s_ = max(y - 1, 0), min(y + 1, h - 1)
        for x in range(w):
            we, ea = max(x - 1, 0), min(x + 1, w - 1)
            adj = F(F(F(p[y, we] + p[y, ea]) + p[n, x]) + p[s_, x])
            diag = F(F(F(p[n, we] + p[n, ea]) + p[s_, we]) + p[s_, ea])
            exp[y, x] = F(F(mult * p[y, x] + F(w1 * mult) * adj) + F(w2 * mult) * diag)
    got = orc.gab1(p, float(w1), float(w2))
    assert np.array_equal(got.view(np.uint32), exp.view(np.uint32))
