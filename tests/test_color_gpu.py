"""Device colour management (jxl_stage_color_convert / jxl_stage_color_peak, csrc/k_color.hip) against the scalar restatement of
the reference in tests/color_ref.py, against its own stages run one by one, against jxl_stage_transfer, and -- at the image
level -- against the host path of JXLImage.transform."""
import ctypes as C
import io
import itertools
import math
import types

import numpy as np
import pytest

import color_ref as ref
from conftest import assert_bits_equal
from jxlatte_amd import _lib, abi, decoder, host
from jxlatte_amd.decoder import (CE_GRAY, CE_RGB, PEAK_DETECT_AUTO, PEAK_DETECT_ON, PRI_BT2100, PRI_P3, PRI_SRGB, TF_BT709, TF_DCI,
                                 TF_LINEAR, TF_PQ, TF_SRGB, WP_D65, DeviceBackend, JXLImage, PNGWriter, UnsupportedOperationException,
                                 get_conversion_matrix)

pytestmark = pytest.mark.gpu
F = np.float32
TF = {"linear": abi.TF_LINEAR, "srgb": abi.TF_SRGB, "bt709": abi.TF_BT709, "pq": abi.TF_PQ, "gamma": abi.TF_GAMMA}
PQ_EDGE = F(math.pow(0.8359375, 1.0 / 0.012683313515655965121))  # ~7.3e-7: below it TF_PQ.toLinear is NaN


def _neighbours(x, k):
    b = int(F(x).view(np.uint32))
    return np.arange(b - k, b + k + 1, dtype=np.int64).astype(np.uint32).view(F)


def _inputs():
    rng = np.random.default_rng(2024)
    edges = np.concatenate([_neighbours(F(0.0404482362771082), 3), _neighbours(F(0.081242858298635133), 3),
                            _neighbours(F(0.018053968510807807), 3), _neighbours(F(0.00313066844250063), 3), _neighbours(PQ_EDGE, 300)])
    special = np.array([0.0, -0.0, -1e-45, -1e-3, -0.5, -2.0, 1.0, 4.0, np.inf, -np.inf, np.nan, 1e-45, 1.1754942e-38, 3.4e38], F)
    return np.concatenate([rng.uniform(0, 1, 700000).astype(F), rng.uniform(1, 4, 100000).astype(F),
                           rng.integers(1, 1 << 23, 100000).astype(np.uint32).view(F), (10 ** rng.uniform(-12, 0, 100000)).astype(F),
                           edges, special])


def _check_curve(got, exp, lin, what):
    """<= 1 float ulp; NaNs, zeros and infinities equal; the linear segment bit for bit. Prints the identical share."""
    special = np.isnan(exp) | np.isnan(got) | (exp == 0) | (got == 0) | np.isinf(exp) | np.isinf(got)
    assert_bits_equal(got[special], exp[special], what + " (NaN / zero / inf lanes)", any_nan=True)
    assert_bits_equal(got[lin], exp[lin], what + " (linear segment)", any_nan=True)
    d = ref.ulp_distance(got[~special], exp[~special])
    print("%s: %.4f %% of %d results bit-identical, max distance %d ulp" % (what, 100.0 * float((d == 0).mean()), d.size, int(d.max())))
    assert int(d.max()) <= 1, what


DIRECTIONS = [("to", "srgb", 0), ("to", "bt709", 0), ("to", "pq", 0), ("to", "gamma", 3846154), ("to", "gamma", 4545455),
              ("to", "gamma", 5555556), ("from", "bt709", 0), ("from", "gamma", 3846154), ("from", "gamma", 4545455),
              ("from", "gamma", 5555556)]


@pytest.mark.parametrize("way,tf,gamma", DIRECTIONS)
def test_each_new_transfer_direction_alone(ctx, way, tf, gamma):
    f = _inputs()
    if way == "to":
        got, = host.colorConvert(ctx, [f], tfIn=TF[tf], gammaIn=gamma)
        exp, lin = ref.to_linear(tf, f, gamma)
    else:
        got, = host.colorConvert(ctx, [f], tfOut=TF[tf], gammaOut=gamma)
        exp, lin = ref.from_linear(tf, f, gamma)
    _check_curve(got, exp, lin, "%s-linear %s %d" % (way, tf, gamma))


def test_zero_of_negative_zero_keeps_math_pow_sign_rules(ctx):
    """Math.pow(-0.0, p) is +0 for a non-integer p; with the integer exponents a gamma header can produce (g = 5000000: p = 2,
    g = 10000000: p = 1 from linear) negative bases follow Math.pow's parity rules"""
    f = np.array([-0.0, 0.0, -2.0, 2.0, -np.inf, np.nan, -0.5], F)
    got, = host.colorConvert(ctx, [f], tfIn=abi.TF_GAMMA, gammaIn=5000000)  # p = 2.0
    assert_bits_equal(got, np.array([0.0, 0.0, 4.0, 4.0, np.inf, np.nan, 0.25], F), "gamma p = 2", any_nan=True)
    got, = host.colorConvert(ctx, [f], tfIn=abi.TF_GAMMA, gammaIn=2000000)  # p = 5.0: odd
    assert_bits_equal(got, np.array([-0.0, 0.0, -32.0, 32.0, -np.inf, np.nan, -0.03125], F), "gamma p = 5", any_nan=True)
    got, = host.colorConvert(ctx, [f], tfIn=abi.TF_GAMMA, gammaIn=4545455)
    assert_bits_equal(got[[0, 1, 4]], np.array([0.0, 0.0, np.inf], F), "gamma p = 2.2 specials")
    assert np.isnan(got[[2, 5, 6]]).all()


@pytest.mark.parametrize("bits", [8, 12, 16])
@pytest.mark.parametrize("tf,gamma", [("srgb", 0), ("bt709", 0), ("pq", 0), ("gamma", 4545455), ("linear", 0)])
def test_every_code_value_of_an_integer_plane(ctx, bits, tf, gamma):
    mx = (1 << bits) - 1
    v = np.arange(mx + 1, dtype=np.int32)
    got, = host.colorConvert(ctx, [v], tfIn=TF[tf], gammaIn=gamma, inMax=[mx])
    exp, lin = ref.to_linear(tf, ref.cast_to_float(v, mx), gamma)
    _check_curve(got, exp, lin, "int%d -> linear from %s" % (bits, tf))
    # transferInPlace's cast: the depth itself as maximum (JXLImage.java:248), bit for bit
    got, = host.colorConvert(ctx, [v], inMax=[bits])
    assert_bits_equal(got, ref.cast_to_float(v, bits), "cast with max = depth")


def _planes(rng, shape, negatives=True):
    p = [rng.uniform(-0.2 if negatives else 0.0, 1.2, shape).astype(F) for _ in range(3)]
    p[0].reshape(-1)[:4] = [0.0, -0.0, np.inf, np.nan]
    return p


def _matrix_np(m, src):
    """decoder.py, JXLImage.toneMapLinear: (m0 a + m1 b) + m2 c in float32"""
    with np.errstate(all="ignore"):
        return [((m[r, 0] * src[0] + m[r, 1] * src[1]).astype(F) + m[r, 2] * src[2]).astype(F) for r in range(3)]


def test_scale_matrix_and_grey_replication_are_exact(ctx):
    rng = np.random.default_rng(7)
    src = _planes(rng, (300, 333))
    for m in (get_conversion_matrix(PRI_SRGB, WP_D65, PRI_P3, WP_D65), get_conversion_matrix(PRI_BT2100, WP_D65, PRI_SRGB, WP_D65)):
        assert not np.array_equal(m, np.eye(3, dtype=F))
        got = host.colorConvert(ctx, src, matrix=m)
        for r, e in enumerate(_matrix_np(m, src)):
            assert_bits_equal(got[r], e, "matrix row %d" % r, any_nan=True)
        grey = host.colorConvert(ctx, src[1:2], matrix=m)
        for r, e in enumerate(_matrix_np(m, [src[1]] * 3)):
            assert_bits_equal(grey[r], e, "grey -> RGB + matrix row %d" % r, any_nan=True)
        # the scale follows the matrix (transform: toneMapLinear, then transfer() with its peak scale)
        s = F(1.7320508)
        both = host.colorConvert(ctx, src, matrix=m, scale=s)
        for r, e in enumerate(_matrix_np(m, src)):
            assert_bits_equal(both[r], (e * s).astype(F), "matrix then scale row %d" % r, any_nan=True)
    for s in (F(1.0000001), F(3.1415927), F(np.nan)):
        got = host.colorConvert(ctx, src, scale=s)
        for c in range(3):
            assert_bits_equal(got[c], (src[c] * s).astype(F), "scale %r plane %d" % (s, c), any_nan=True)
    one, = host.colorConvert(ctx, src[:1], scale=F(0.3))
    assert_bits_equal(one, (src[0] * F(0.3)).astype(F), "grey scale", any_nan=True)


def _peak_planes():
    rng = np.random.default_rng(5)
    nan = np.nan
    out = {}
    for name, shape in (("1x1", (1, 1)), ("row", (1, 777)), ("column", (301, 1)), ("odd", (37, 1000)), ("wide", (5, 70001))):
        out[name] = rng.uniform(-1, 2, shape).astype(F)
    a = rng.uniform(0, 1, (9, 130)).astype(F)
    a[3, 0] = nan                      # first of a row: sticks
    out["nan-first"] = a
    b = rng.uniform(0, 1, (9, 130)).astype(F)
    b[2, 1] = nan
    b[4, 129] = nan
    b[5, 64:70] = nan                  # elsewhere: passed over
    out["nan-elsewhere"] = b
    out["all-nan"] = np.full((4, 65), nan, F)
    z = np.zeros((6, 200), F)
    z[0, :] = 0.0
    z[0, 100] = -0.0                   # +0 first: stays +0
    z[1, :] = -0.0
    z[1, 3] = 0.0                      # -0 first: stays -0
    z[2:, :] = -1.0                    # lower rows: the row results are -1
    out["zeros"] = z
    z2 = np.full((3, 300), 5.0, F)
    z2[0, 299] = -0.0
    z2[1, 0] = 0.0
    z2[2, 150] = -0.0
    z2[2, 151] = 0.0
    out["zero-rows"] = z2              # row results -0, +0, -0: the maximum is +0
    z3 = z2.copy()
    z3[1, 0] = 5.0
    z3[1, 7] = -0.0
    out["negative-zero-rows"] = z3     # every row -0
    out["inf"] = np.array([[np.inf, nan], [np.inf, np.inf], [-np.inf, 1]], F)
    return out


@pytest.mark.parametrize("name", sorted(_peak_planes()))
def test_peak_equals_the_serial_definition(ctx, name):
    plane = _peak_planes()[name]
    exp = ref.determine_peak(plane)
    assert_bits_equal(np.array([host.determinePeak(ctx, [plane])], F), np.array([exp], F), "grey " + name, any_nan=True)
    other = np.full(plane.shape, 9.0, F)
    assert_bits_equal(np.array([host.determinePeak(ctx, [other, plane, other])], F), np.array([exp], F), "green " + name, any_nan=True)


def test_peak_of_integer_and_transformed_planes(ctx):
    rng = np.random.default_rng(6)
    v = rng.integers(0, 4000, (130, 259)).astype(np.int32)
    assert_bits_equal(np.array([host.determinePeak(ctx, [v], inMax=[4095])], F), np.array([ref.determine_peak(v, 4095)], F), "int plane")
    z = np.zeros((3, 5), np.int32)
    assert_bits_equal(np.array([host.determinePeak(ctx, [z, z, z], inMax=[255] * 3)], F), np.array([0.0], F), "int zeros")
    # a tagged plane: the peak is that of the linearised samples (same front stages as color_convert, nothing stored between)
    lin, = host.colorConvert(ctx, [v], tfIn=abi.TF_SRGB, inMax=[4095])
    assert_bits_equal(np.array([host.determinePeak(ctx, [v], tfIn=abi.TF_SRGB, inMax=[4095])], F), np.array([ref.determine_peak(lin)], F), "sRGB int plane")
    pq = rng.uniform(0, 1, (50, 70)).astype(F)
    pq[:, 0] = 0.0  # PQ of zero is NaN: first of every row
    lin, = host.colorConvert(ctx, [pq], tfIn=abi.TF_PQ)
    assert np.isnan(lin[:, 0]).all() and np.isnan(host.determinePeak(ctx, [pq], tfIn=abi.TF_PQ))
    # after a matrix: row 1 of it (toneMapLinear runs before transfer() takes the peak)
    src = [rng.uniform(0, 1, (40, 90)).astype(F) for _ in range(3)]
    m = get_conversion_matrix(PRI_SRGB, WP_D65, PRI_BT2100, WP_D65)
    mapped = host.colorConvert(ctx, src, tfIn=abi.TF_PQ, matrix=m)
    got = host.determinePeak(ctx, src, tfIn=abi.TF_PQ, matrix=m)
    assert_bits_equal(np.array([got], F), np.array([ref.determine_peak(mapped[1])], F), "peak after the matrix", any_nan=True)


def _staged(ctx, planes, tf_in, gamma_in, in_max, scale, matrix, tf_out, gamma_out, max_value):
    """the same chain as separate calls with float intermediates"""
    cur = list(planes)
    if cur[0].dtype == np.int32:
        cur = host.colorConvert(ctx, cur, inMax=in_max)
    if tf_in != abi.TF_LINEAR:
        cur = host.colorConvert(ctx, cur, tfIn=tf_in, gammaIn=gamma_in)
    if matrix is not None:
        cur = host.colorConvert(ctx, cur, matrix=matrix)
    if scale is not None:
        cur = host.colorConvert(ctx, cur, scale=scale)
    linear = cur
    if tf_out != abi.TF_LINEAR or max_value:
        cur = host.colorConvert(ctx, cur, tfOut=tf_out, gammaOut=gamma_out, maxValue=max_value)
    return cur, linear


GRID_TF = [(abi.TF_LINEAR, 0), (abi.TF_SRGB, 0), (abi.TF_BT709, 0), (abi.TF_PQ, 0), (abi.TF_GAMMA, 4545455)]


@pytest.mark.parametrize("tf_in,gamma_in", GRID_TF)
def test_fused_equals_staged(ctx, tf_in, gamma_in):
    rng = np.random.default_rng(100 + tf_in)
    shape = (24, 173)
    m = get_conversion_matrix(PRI_SRGB, WP_D65, PRI_P3, WP_D65)
    f3 = _planes(rng, shape)
    i3 = [rng.integers(0, 256, shape).astype(np.int32) for _ in range(3)]
    n = 0
    for (tf_out, gamma_out), use_scale, use_matrix, max_value, grey, is_int in itertools.product(
            GRID_TF, (False, True), (False, True), (0, 255, 65535), (False, True), (False, True)):
        planes = (i3 if is_int else f3)[:1 if grey else 3]
        kw = dict(tf_in=tf_in, gamma_in=gamma_in, in_max=[255] * len(planes), scale=F(1.37) if use_scale else None,
                  matrix=m if use_matrix else None, tf_out=tf_out, gamma_out=gamma_out, max_value=max_value)
        fused = host.colorConvert(ctx, planes, tfIn=tf_in, gammaIn=gamma_in, inMax=kw["in_max"], scale=kw["scale"], matrix=kw["matrix"],
                                  tfOut=tf_out, gammaOut=gamma_out, maxValue=max_value)
        staged, linear = _staged(ctx, planes, **kw)
        what = "in %d out %d scale %d matrix %d max %d grey %d int %d" % (tf_in, tf_out, use_scale, use_matrix, max_value, grey, is_int)
        assert len(fused) == len(staged) == (1 if grey and not use_matrix else 3), what
        for c in range(len(fused)):
            assert_bits_equal(fused[c], staged[c], what + " plane %d" % c, any_nan=True)
            if tf_out in (abi.TF_PQ, abi.TF_SRGB):  # the tail is jxl_stage_transfer's
                code = abi.TRANSFER_PQ if tf_out == abi.TF_PQ else abi.TRANSFER_SRGB
                assert_bits_equal(fused[c], host.transfer(ctx, linear[c], code, max_value), what + " vs jxl_stage_transfer, plane %d" % c, any_nan=True)
        n += 1
    assert n == 5 * 2 * 2 * 3 * 2 * 2


def _info(gray=False, bits=8, transfer=TF_SRGB, prim=PRI_SRGB):
    return types.SimpleNamespace(colour_space=CE_GRAY if gray else CE_RGB, num_extra=0, ec_type=[], ec_alpha_associated=[], ec_bits=[],
                                 prim_xy=list(prim), white_xy=list(WP_D65), transfer=transfer, xyb_encoded=False,
                                 bits_per_sample=bits, use_icc=False)


@pytest.fixture(scope="module")
def backend(ctx):
    be = DeviceBackend.__new__(DeviceBackend)
    be.host, be.ctx = host, ctx
    return be


def _image_cases():
    rng = np.random.default_rng(42)
    shape = (96, 160)
    # rows of nearly constant level: determinePeak takes each row's MINIMUM, so that only such rows leave samples below the peak
    level = rng.uniform(0.2, 0.6, (shape[0], 1))
    pq = [(level + rng.uniform(-0.01, 0.01, shape)).astype(F) for _ in range(3)]
    dark = [p.copy() for p in pq]
    for p in dark:
        p[:, 0] = 0.0
    return {
        "p3-int8": ([rng.integers(0, 256, shape).astype(np.int32) for _ in range(3)], _info(prim=PRI_P3), False),
        "bt709-float": ([rng.uniform(0, 1, shape).astype(F) for _ in range(3)], _info(transfer=TF_BT709, bits=16), False),
        "pq-bt2100": (pq, _info(transfer=TF_PQ, prim=PRI_BT2100, bits=16), False),
        "pq-bt2100-dark-column": (dark, _info(transfer=TF_PQ, prim=PRI_BT2100, bits=16), False),
        "pq-bt2100-as-hdr": (pq, _info(transfer=TF_PQ, prim=PRI_BT2100, bits=16), True),
        "grey-gamma-int16": ([rng.integers(0, 65536, shape).astype(np.int32)], _info(gray=True, bits=16, transfer=4545455, prim=PRI_P3), False),
        "grey-gamma-int16-same-primaries": ([rng.integers(0, 65536, shape).astype(np.int32)], _info(gray=True, bits=16, transfer=4545455), False),
    }


def _meta(im):
    return (im.transfer_, [float(v) for v in im.primariesXY], [float(v) for v in im.whiteXY], im.colorEncoding, list(im.bitDepths),
            len(im.buffer), [b.dtype for b in im.buffer], [b.shape for b in im.buffer])


@pytest.mark.parametrize("name", sorted(_image_cases()))
def test_png_writer_device_colour(ctx, backend, name):
    buf, info, hdr = _image_cases()[name]
    im = JXLImage([b.copy() for b in buf], info, backend)
    prim, tf = (PRI_BT2100, TF_PQ) if hdr else (PRI_SRGB, TF_SRGB)
    dev = PNGWriter(im, hdr=hdr, deviceColor=True)
    hst = PNGWriter(im, hdr=hdr)
    # (a) metadata
    a, b = im.transform(prim, WP_D65, tf, PEAK_DETECT_AUTO, device=True), im.transform(prim, WP_D65, tf, PEAK_DETECT_AUTO)
    assert _meta(a) == _meta(b)
    assert (dev.bitDepth, dev.colorMode, dev.width, dev.height) == (hst.bitDepth, hst.colorMode, hst.width, hst.height)
    # (b) the staged device calls
    colors = len(buf)
    tone_map = not decoder._prim_matches(prim, im.primariesXY)
    m = get_conversion_matrix(prim, WP_D65, im.primariesXY, im.whiteXY) if tone_map else None
    tf_in, gamma_in = decoder._tf_selector(info.transfer)
    tf_out, _ = decoder._tf_selector(tf)
    depth_max = [(1 << info.bits_per_sample) - 1] * colors
    scale = None
    if tf != info.transfer or tone_map:
        front, _ = _staged(ctx, buf, tf_in, gamma_in, depth_max, None, m, abi.TF_LINEAR, 0, 0)
        if info.transfer == TF_PQ and tf == TF_SRGB:
            peak = host.determinePeak(ctx, front)
            s = F(F(1) / peak)
            print("%s: peak %r" % (name, peak))
            assert np.isnan(peak) == ("dark" in name)
            scale = s if s > 1.0 else None
        staged, _ = _staged(ctx, buf, tf_in, gamma_in, depth_max, scale, m, tf_out, 0, 0)
        for c in range(len(staged)):
            assert_bits_equal(a.buffer[c], staged[c], name + " plane %d vs staged" % c, any_nan=True)
    else:
        assert a is im
    # (c) at most one code value from the host path's PNG; the count is reported
    d = np.abs(dev.samples.astype(np.int64) - hst.samples.astype(np.int64))
    print("%s: %d of %d PNG samples differ from the host path (max %d)" % (name, int((d != 0).sum()), d.size, int(d.max())))
    assert int(d.max()) <= 1
    out = io.BytesIO()
    dev.write(out)
    assert out.getvalue()[:8] == b"\x89PNG\r\n\x1a\n"


def test_peak_detect_on_scales_even_below_one(backend):
    rng = np.random.default_rng(9)
    buf = [rng.uniform(0.6, 0.9, (20, 30)).astype(F) for _ in range(3)]
    im = JXLImage(buf, _info(transfer=TF_PQ, bits=16), backend)
    auto = im.transform(PRI_SRGB, WP_D65, TF_LINEAR, PEAK_DETECT_AUTO, device=True)
    lin = host.colorConvert(backend.ctx, buf, tfIn=abi.TF_PQ)
    for c in range(3):
        assert_bits_equal(auto.buffer[c], lin[c], "to linear: no peak")
    peak = host.determinePeak(backend.ctx, buf, tfIn=abi.TF_PQ)
    on = im.transform(PRI_SRGB, WP_D65, TF_BT709, PEAK_DETECT_ON, device=True)
    exp = host.colorConvert(backend.ctx, buf, tfIn=abi.TF_PQ, scale=F(F(1) / peak), tfOut=abi.TF_BT709)
    for c in range(3):
        assert_bits_equal(on.buffer[c], exp[c], "peak detect on")


def test_bt709_dci_and_gamma_targets_work_on_the_device_path(backend):
    rng = np.random.default_rng(10)
    buf = [rng.uniform(0, 1, (33, 65)).astype(F) for _ in range(3)]
    im = JXLImage(buf, _info(transfer=TF_LINEAR, bits=16), backend)
    for target, (way, tf, gamma) in ((TF_BT709, ("from", "bt709", 0)), (TF_DCI, ("from", "gamma", 3846154)), (4545455, ("from", "gamma", 4545455))):
        with pytest.raises(UnsupportedOperationException):
            im.transform(PRI_SRGB, WP_D65, target)
        out = im.transform(PRI_SRGB, WP_D65, target, device=True)
        assert out.transfer_ == target and len(out.buffer) == 3
        for c in range(3):
            exp, lin = ref.from_linear(tf, buf[c], gamma)
            _check_curve(out.buffer[c], exp, lin, "target %d plane %d" % (target, c))


def _call(ctx, in_planes, n, p, out_planes):
    pin = (C.c_void_p * 3)(*[a.ctypes.data if a is not None else None for a in in_planes])
    pout = (C.c_void_p * 3)(*[a.ctypes.data if a is not None else None for a in out_planes])
    return ctx.lib.jxl_stage_color_convert(ctx.h, pin, n, C.byref(p) if p is not None else None, pout)


def test_argument_checks(ctx):
    src = [np.full(64, 0.5, F) for _ in range(3)]
    out = [np.full(64, -7.0, F) for _ in range(3)]

    def params(**kw):
        p = host.colorParams(src)
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    bad = [params(tf_in=9), params(tf_in=-1), params(tf_out=6), params(tf_in=abi.TF_GAMMA, gamma_in=0),
           params(tf_in=abi.TF_GAMMA, gamma_in=1 << 24), params(tf_out=abi.TF_GAMMA, gamma_out=-5), params(n_planes=2), params(n_planes=0),
           params(max_value=-1), params(in_is_int=1)]  # (in_max = 0)
    for p in bad:
        assert _call(ctx, src, 64, p, out) == abi.JXL_ERR_INVALID_ARGUMENT
    for p in (params(tf_in=abi.TF_HLG), params(tf_out=abi.TF_HLG)):
        assert _call(ctx, src, 64, p, out) == abi.JXL_ERR_UNSUPPORTED
    assert _call(ctx, [src[0], None, src[2]], 64, params(), out) == abi.JXL_ERR_INVALID_ARGUMENT
    assert _call(ctx, src, 64, params(), [out[0], out[1], None]) == abi.JXL_ERR_INVALID_ARGUMENT
    assert _call(ctx, src, -1, params(), out) == abi.JXL_ERR_INVALID_ARGUMENT
    assert _call(ctx, src, 64, None, out) == abi.JXL_ERR_INVALID_ARGUMENT
    # a matrix has three planes to write: a grey output of it cannot be asked for
    grey = params(n_planes=1, use_matrix=1)
    assert _call(ctx, [src[0], None, None], 64, grey, [out[0], None, None]) == abi.JXL_ERR_INVALID_ARGUMENT
    assert all(np.all(o == F(-7.0)) for o in out), "a rejected call wrote"
    assert _call(ctx, src, 0, params(), out) == abi.JXL_OK and all(np.all(o == F(-7.0)) for o in out)  # n = 0: nothing
    assert _call(ctx, [src[0], None, None], 64, grey, out) == abi.JXL_OK and all(np.all(o == F(0.0)) for o in out)  # zero matrix
    with pytest.raises(_lib.UnsupportedOperationException):
        host.colorConvert(ctx, src, tfIn=abi.TF_HLG)
    peak = C.c_float(-7.0)
    pin = (C.c_void_p * 3)(*[a.ctypes.data for a in src])
    for h, w, p in ((0, 64, params()), (8, 0, params()), (8, 8, params(tf_in=17)), (8, 8, params(n_planes=2))):
        assert ctx.lib.jxl_stage_color_peak(ctx.h, pin, h, w, C.byref(p), C.byref(peak)) == abi.JXL_ERR_INVALID_ARGUMENT
    assert ctx.lib.jxl_stage_color_peak(ctx.h, pin, 8, 8, C.byref(params(tf_in=abi.TF_HLG)), C.byref(peak)) == abi.JXL_ERR_UNSUPPORTED
    assert peak.value == -7.0
