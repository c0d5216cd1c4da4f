"""The PNG's samples in one device pass (jxl_stage_png_samples / jxl_planes_png_samples, csrc/k_png.hip) against the two-pass
path it replaces (jxl_stage_color_convert with float output, then jxl_stage_pack: existing code), against a numpy float32
restatement where no pow is involved, against tests/color_ref.py's curves for the sRGB and PQ targets; the group-of-4 tail; the
argument checks; and the resident-plane entries (jxl_planes_orient, jxl_planes_color_peak)."""
import ctypes as C
import itertools
import math

import numpy as np
import pytest

import color_ref as ref
from conftest import assert_bits_equal
from jxlatte_amd import _lib, abi, host
from jxlatte_amd.decoder import PRI_BT2100, PRI_P3, PRI_SRGB, WP_D65, get_conversion_matrix

pytestmark = pytest.mark.gpu
F = np.float32
N = 4099  # no multiple of 4: the last lane takes the sample-by-sample path
PQ_EDGE = F(math.pow(0.8359375, 1.0 / 0.012683313515655965121))
GRID_TF = [(abi.TF_LINEAR, 0), (abi.TF_SRGB, 0), (abi.TF_BT709, 0), (abi.TF_PQ, 0), (abi.TF_GAMMA, 4545455)]
MATRIX = get_conversion_matrix(PRI_SRGB, WP_D65, PRI_P3, WP_D65)


def _neighbours(x, k):
    b = int(F(x).view(np.uint32))
    return np.arange(b - k, b + k + 1, dtype=np.int64).astype(np.uint32).view(F)


def _float_plane(seed):
    """test_color_gpu._inputs() in small: the uniform ranges, the curves' break points +- 3 ulp, the special values"""
    rng = np.random.default_rng(seed)
    edges = np.concatenate([_neighbours(F(0.0404482362771082), 3), _neighbours(F(0.081242858298635133), 3),
                            _neighbours(F(0.018053968510807807), 3), _neighbours(F(0.00313066844250063), 3), _neighbours(PQ_EDGE, 3)])
    special = np.array([0.0, -0.0, -1e-45, -1e-3, -0.5, -2.0, 1.0, 4.0, np.inf, -np.inf, np.nan, 1e-45, 1.1754942e-38, 3.4e38], F)
    k = N - edges.size - special.size
    body = np.concatenate([rng.uniform(0, 1, k - 600).astype(F), rng.uniform(1, 4, 200).astype(F),
                           rng.integers(1, 1 << 23, 200).astype(np.uint32).view(F), (10 ** rng.uniform(-12, 0, 200)).astype(F)])
    v = np.concatenate([body, edges, special])
    rng.shuffle(v)
    assert v.size == N
    return v.reshape(1, N)


def _int_plane(seed, mx=255):
    rng = np.random.default_rng(seed)
    v = rng.integers(0, mx + 1, N).astype(np.int32)
    v[:8] = [0, mx, mx + 1, -1, -300, 2 ** 31 - 1, -2 ** 31, 1]
    rng.shuffle(v)
    return v.reshape(1, N)


def _alpha(kind, seed, mx=255):
    rng = np.random.default_rng(seed)
    if kind == "float":
        a = rng.uniform(0, 1, N).astype(F)
        a[:8] = [0.0, -0.0, 1.0, 1.5, np.nan, np.inf, 0.5, 1e-30]
    else:
        a = rng.integers(0, mx + 1, N).astype(np.int32)
        a[:6] = [0, mx, mx + 45, -1, 1, 2 ** 31 - 1]
    rng.shuffle(a)
    return a.reshape(1, N)


@pytest.fixture(scope="module")
def planes():
    return dict(f=[_float_plane(s) for s in (1, 2, 3)], i=[_int_plane(s) for s in (4, 5, 6)],
                alpha=dict(float=_alpha("float", 7), int=_alpha("int", 8)))


# (alpha kind or None, premultiplied)
ALPHAS = [(None, False), ("float", False), ("float", True), ("int", False), ("int", True)]


def _staged_pack(ctx, colour, alpha, premultiplied, depth, alpha_depth, big_endian=True):
    tagged = [depth] * len(colour) + ([alpha_depth] if alpha is not None else [])
    tagged += [depth] * (4 - len(tagged))
    return host.packSamples(ctx, colour, depth, alpha=alpha, premultiplied=premultiplied, taggedDepth=tagged, bigEndian=big_endian)


@pytest.mark.parametrize("tf_in,gamma_in", GRID_TF)
def test_fused_equals_staged_byte_for_byte(ctx, planes, tf_in, gamma_in):
    """tf_in x tf_out x scale x matrix x grey x int (test_color_gpu's grid; max_value is 0 here by definition) x {8, 16 bit} x
    {no alpha, straight, premultiplied} x {float, int alpha}: the bytes of colorConvert(maxValue=0) + packSamples"""
    n = 0
    for (tf_out, gamma_out), use_scale, use_matrix, grey, is_int in itertools.product(GRID_TF, (False, True), (False, True), (False, True), (False, True)):
        src = (planes["i"] if is_int else planes["f"])[:1 if grey else 3]
        kw = dict(tfIn=tf_in, gammaIn=gamma_in, inMax=[255] * len(src), scale=F(1.37) if use_scale else None,
                  matrix=MATRIX if use_matrix else None, tfOut=tf_out, gammaOut=gamma_out)
        colour = host.colorConvert(ctx, src, maxValue=0, **kw)
        for depth, (akind, premult) in itertools.product((8, 16), ALPHAS):
            alpha = planes["alpha"][akind] if akind else None
            exp = _staged_pack(ctx, colour, alpha, premult, depth, 8)
            got = host.pngSamples(ctx, src, alpha, premultiplied=premult, bitDepth=depth, bigEndian=True, alphaDepth=8, **kw)
            what = "in %d out %d scale %d matrix %d grey %d int %d depth %d alpha %s premult %d" % (
                tf_in, tf_out, use_scale, use_matrix, grey, is_int, depth, akind, premult)
            assert got.dtype == exp.dtype and got.shape == exp.shape, what
            assert np.array_equal(got, exp), what + ": %d samples differ" % int((got != exp).sum())
            n += 1
    assert n == 5 * 2 * 2 * 2 * 2 * 2 * 5
    # host byte order, and an int alpha of the PNG's own depth (not coerced: clamped as it is)
    for depth, big in ((16, False), (8, False)):
        alpha = _alpha("int", 9, (1 << depth) - 1)
        colour = host.colorConvert(ctx, planes["f"], tfIn=tf_in, gammaIn=gamma_in)
        exp = _staged_pack(ctx, colour, alpha, False, depth, depth, big_endian=big)
        got = host.pngSamples(ctx, planes["f"], alpha, bitDepth=depth, bigEndian=big, alphaDepth=depth, tfIn=tf_in, gammaIn=gamma_in)
        assert np.array_equal(got, exp), "little-endian / uncoerced alpha, depth %d" % depth


LAYOUTS = [("rgb8", 3, False, 8), ("rgba8", 3, True, 8), ("rgb16", 3, False, 16), ("rgba16", 3, True, 16), ("grey8", 1, False, 8),
           ("greya8", 1, True, 8), ("grey16", 1, False, 16), ("greya16", 1, True, 16)]


def _call_stage(ctx, src, alpha, p, out):
    pin = (C.c_void_p * 3)(*([a.ctypes.data if a is not None else None for a in src] + [None] * (3 - len(src))))
    return ctx.lib.jxl_stage_png_samples(ctx.h, pin, alpha.ctypes.data if alpha is not None else None, C.byref(p) if p is not None else None,
                                         out.ctypes.data if out is not None else None)


@pytest.mark.parametrize("name,colors,has_alpha,depth", LAYOUTS)
def test_group_of_four_tail_writes_nothing_behind_the_last_sample(ctx, name, colors, has_alpha, depth):
    rng = np.random.default_rng(11)
    for n in (1, 2, 3, 4, 5, 7, 8, 1023, 1025):
        src = [rng.uniform(-0.1, 1.1, (1, n)).astype(F) for _ in range(colors)]
        alpha = rng.uniform(0.2, 1, (1, n)).astype(F) if has_alpha else None
        p = host.pngParams(src, (1, n), alpha=alpha, bitDepth=depth, bigEndian=True, tfOut=abi.TF_SRGB)
        nbytes = n * (colors + has_alpha) * depth // 8
        out = np.full(nbytes + 64, 0xA5, np.uint8)
        assert _call_stage(ctx, src, alpha, p, out) == abi.JXL_OK
        assert np.all(out[nbytes:] == 0xA5), "%s n %d: bytes behind the last sample were written" % (name, n)
        colour = host.colorConvert(ctx, src, tfOut=abi.TF_SRGB)
        exp = _staged_pack(ctx, colour, alpha, False, depth, depth)
        assert np.array_equal(out[:nbytes], exp.reshape(-1).view(np.uint8)), "%s n %d" % (name, n)
        # the same with the guard where the kernel stores: 64 bytes behind the samples in the DEVICE buffer come down too
        dev = np.zeros(nbytes + 64, np.uint8)
        pin = (C.c_void_p * 3)(*([a.ctypes.data for a in src] + [None] * (3 - len(src))))
        guard = ctx.lib.jxl_debug_png_samples_guard
        guard.restype, guard.argtypes = C.c_int32, [C.c_void_p, C.POINTER(C.c_void_p), C.c_void_p, C.POINTER(abi.PngParams), C.c_void_p, C.c_int32]
        assert guard(ctx.h, pin, alpha.ctypes.data if alpha is not None else None, C.byref(p), dev.ctypes.data, 64) == abi.JXL_OK
        assert np.all(dev[nbytes:] == 0xA5), "%s n %d: the kernel stored behind the last sample" % (name, n)
        assert np.array_equal(dev[:nbytes], out[:nbytes]), "%s n %d (device guard run)" % (name, n)


def _java_int(v):
    """(int)float: NaN -> 0, saturating"""
    with np.errstate(all="ignore"):
        d = np.nan_to_num(v.astype(np.float64), nan=0.0, posinf=2.0 ** 31, neginf=-2.0 ** 31)
    return np.clip(np.trunc(d), -2.0 ** 31, 2.0 ** 31 - 1).astype(np.int64)


def _quant(v, maxv):
    with np.errstate(all="ignore"):
        return np.clip(_java_int((v * F(maxv)).astype(F) + F(0.5)), 0, maxv)


def _numpy_samples(src, in_max, matrix, scale, alpha, premult, depth, alpha_depth):
    """the float32 operations of the stages without a pow, restated: cast, matrix, scale, coercion, division, quantiser"""
    maxv = (1 << depth) - 1
    with np.errstate(all="ignore"):
        v = [ref.cast_to_float(a, in_max) if a.dtype == np.int32 else a for a in src]
        if matrix is not None:
            v = v * 3 if len(v) == 1 else v
            v = [((matrix[r, 0] * v[0] + matrix[r, 1] * v[1]).astype(F) + matrix[r, 2] * v[2]).astype(F) for r in range(3)]
        if scale is not None:
            v = [(a * F(scale)).astype(F) for a in v]
        cols = []
        fa = None
        if alpha is not None:
            coerce = premult or (alpha.dtype == np.int32 and alpha_depth != depth)
            if alpha.dtype == np.int32 and not coerce:
                qa = np.clip(alpha.astype(np.int64), 0, maxv)
            else:
                fa = ref.cast_to_float(alpha, (1 << alpha_depth) - 1) if alpha.dtype == np.int32 else alpha
                qa = _quant(fa, maxv)
            if premult:
                v = [(a / fa).astype(F) for a in v]
        cols = [_quant(a, maxv) for a in v] + ([qa] if alpha is not None else [])
    out = np.stack(cols, axis=-1).astype(np.uint8 if depth == 8 else np.uint16)
    return out.byteswap() if depth == 16 else out  # big-endian samples, as the writer wants them


def test_stages_without_a_pow_equal_numpy_float32(ctx, planes):
    """independent of the existing kernels: int8 / int16 / float input, linear in and out, with and without matrix and scale,
    no / straight / premultiplied alpha (float and int), 8 and 16 bit"""
    i16 = [_int_plane(s, 65535) for s in (21, 22, 23)]
    inputs = [("float", planes["f"], 255), ("int8", planes["i"], 255), ("int16", i16, 65535)]
    n = 0
    for (iname, src3, in_max), grey, use_matrix, use_scale, depth, (akind, premult) in itertools.product(
            inputs, (False, True), (False, True), (False, True), (8, 16), ALPHAS):
        src = src3[:1 if grey else 3]
        m = MATRIX if use_matrix else None
        s = F(0.8125) if use_scale else None
        alpha = planes["alpha"][akind] if akind else None
        got = host.pngSamples(ctx, src, alpha, premultiplied=premult, bitDepth=depth, bigEndian=True, alphaDepth=8,
                              inMax=[in_max] * len(src), matrix=m, scale=s)
        exp = _numpy_samples(src, in_max, m, s, alpha, premult, depth, 8)
        what = "%s grey %d matrix %d scale %d depth %d alpha %s premult %d" % (iname, grey, use_matrix, use_scale, depth, akind, premult)
        assert got.shape == exp.shape and np.array_equal(got, exp), what + ": %d samples differ" % int((got != exp).sum())
        n += 1
    assert n == 3 * 2 * 2 * 2 * 2 * 5


def _from_linear_ref(tf, f):
    """TransferFunction.fromLinearF of the two PNG targets, which tests/color_ref.py leaves to jxl_stage_transfer's own tests:
    restated with its Math.pow stand-in (color_ref.jpow) and float32 roundings where the Java code rounds to float"""
    d = f.astype(np.float64)
    with np.errstate(all="ignore"):
        if tf == "srgb":  # TransferFunction.java:39-44
            curve = ((F(1.055) * ref.jpow(d, 0.4166666666666667).astype(F)).astype(F) + F(-0.055)).astype(F)
            return np.where(f < F(0.00313066844250063), (f * F(12.92)).astype(F), curve)
        e = ref.jpow(d, 0.159423828125)  # :83-87, the interface's (float)fromLinear((double)f)
        return ref.jpow((0.8359375 + 18.8515625 * e) / (1.0 + 18.6875 * e), 78.84375).astype(F)


@pytest.mark.parametrize("tf", ["srgb", "pq"])
@pytest.mark.parametrize("depth", [8, 16])
def test_srgb_and_pq_targets_within_one_code_value_of_the_reference_curve(ctx, planes, tf, depth):
    """the reference's curve, (float)Math.pow forms through tests/color_ref.py's pow, followed by the same quantiser. The curves are within 1 float ulp of the
    reference (include/jxlatte_amd.h); through the quantiser that is at most one code value."""
    src = planes["f"]
    got = host.pngSamples(ctx, src, None, bitDepth=depth, bigEndian=False, tfOut={"srgb": abi.TF_SRGB, "pq": abi.TF_PQ}[tf])
    maxv = (1 << depth) - 1
    exp = np.stack([_quant(_from_linear_ref(tf, a), maxv) for a in src], axis=-1)
    d = np.abs(got.astype(np.int64) - exp)
    print("%s %d bit: %d of %d samples differ from the reference curve (max %d)" % (tf, depth, int((d != 0).sum()), d.size, int(d.max())))
    assert int(d.max()) <= 1


def test_argument_checks(ctx):
    src = [np.full((4, 16), 0.5, F) for _ in range(3)]
    alpha = np.full((4, 16), 1.0, F)
    out = np.full(4 * 16 * 4 * 2, 0xA5, np.uint8)

    def params(color=None, **kw):
        p = host.pngParams(src, (4, 16), alpha=alpha)
        for k, v in (color or {}).items():
            setattr(p.color, k, v)
        for k, v in kw.items():
            setattr(p, k, v)
        return p
    bad = [params(color=dict(max_value=255)), params(bit_depth=12), params(color=dict(n_planes=2)), params(height=-4), params(width=-16),
           params(height=0), params(premultiplied=1, has_alpha=0), params(color=dict(tf_out=9)), params(color=dict(in_is_int=1), color_tagged_depth=0),
           params(alpha_is_int=1, premultiplied=1, alpha_tagged_depth=0)]
    for p in bad:
        assert _call_stage(ctx, src, alpha, p, out) == abi.JXL_ERR_INVALID_ARGUMENT
    assert _call_stage(ctx, [src[0], None, src[2]], alpha, params(), out) == abi.JXL_ERR_INVALID_ARGUMENT  # a missing plane
    assert _call_stage(ctx, src, None, params(), out) == abi.JXL_ERR_INVALID_ARGUMENT  # the alpha plane it announces
    assert _call_stage(ctx, src, alpha, None, out) == abi.JXL_ERR_INVALID_ARGUMENT
    assert _call_stage(ctx, src, alpha, params(), None) == abi.JXL_ERR_INVALID_ARGUMENT
    assert _call_stage(ctx, src, alpha, params(color=dict(tf_in=abi.TF_HLG)), out) == abi.JXL_ERR_UNSUPPORTED
    assert np.all(out == 0xA5), "a rejected call wrote"
    assert _call_stage(ctx, src, alpha, params(), out) == abi.JXL_OK and np.all(out[:4 * 16 * 4] != 0xA5)
    # the resident entries on a context that has no resident planes
    with _lib.Context(ctx.device) as fresh:
        p = params()
        peak = C.c_float(-7.0)
        assert fresh.lib.jxl_planes_png_samples(fresh.h, None, C.byref(p), out.ctypes.data) == abi.JXL_ERR_STATE
        assert fresh.lib.jxl_planes_color_peak(fresh.h, C.byref(p.color), C.byref(peak)) == abi.JXL_ERR_STATE
        assert fresh.lib.jxl_planes_orient(fresh.h, 3) == abi.JXL_ERR_STATE
        assert peak.value == -7.0
        with pytest.raises(_lib.IllegalStateException):
            host.ResidentPlanes(fresh).pngSamples()
        # with planes: a geometry other than theirs, an orientation out of range
        rp = host.ResidentPlanes.upload(fresh, np.zeros((3, 4, 16), F))
        assert fresh.lib.jxl_planes_png_samples(fresh.h, alpha.ctypes.data, C.byref(params(height=16, width=4)), out.ctypes.data) == abi.JXL_ERR_INVALID_ARGUMENT
        assert fresh.lib.jxl_planes_orient(fresh.h, 9) == abi.JXL_ERR_STATE and rp.shape == (4, 16)


@pytest.fixture(scope="module")
def resident_src():
    rng = np.random.default_rng(31)
    pl = rng.uniform(0.05, 0.9, (3, 37, 53)).astype(F)
    pl[1, :, 0] = np.nan        # a NaN first column (of the unoriented planes)
    pl[1, 5, :] = -0.0          # a row of zeros of both signs
    pl[1, 5, 7] = 0.0
    pl[1, 3, 0] = 0.25
    return pl


@pytest.mark.parametrize("o", range(1, 9))
def test_resident_orient_equals_the_stage(ctx, resident_src, o):
    rp = host.ResidentPlanes.upload(ctx, resident_src)
    rp.orient(o)
    got = rp.download()
    exp = np.stack([host.transposeBuffer(ctx, resident_src[c], o) for c in range(3)])
    assert rp.shape == exp.shape[1:] == ((53, 37) if o > 4 else (37, 53))
    assert_bits_equal(got, exp, "orientation %d" % o, any_nan=True)


def test_resident_peak_and_samples_equal_the_stage_entries(ctx, resident_src):
    m = get_conversion_matrix(PRI_SRGB, WP_D65, PRI_BT2100, WP_D65)
    for o in (1, 6):
        rp = host.ResidentPlanes.upload(ctx, resident_src)
        rp.orient(o)
        down = [np.ascontiguousarray(a) for a in rp.download()]
        for front in (dict(), dict(tfIn=abi.TF_SRGB), dict(tfIn=abi.TF_PQ, matrix=m)):
            got, exp = rp.colorPeak(**front), host.determinePeak(ctx, down, **front)
            assert_bits_equal(np.array([got], F), np.array([exp], F), "peak, orientation %d, %r" % (o, sorted(front)), any_nan=True)
        # (the plain peak is the serial definition's, NaN column and zero row included)
        assert_bits_equal(np.array([rp.colorPeak()], F), np.array([ref.determine_peak(down[1])], F), "peak vs color_ref, orientation %d" % o, any_nan=True)
        alpha = np.random.default_rng(o).uniform(0, 1, rp.shape).astype(F)
        for kw in (dict(bitDepth=8, tfOut=abi.TF_SRGB), dict(bitDepth=16, tfIn=abi.TF_PQ, matrix=m, scale=F(1.5), tfOut=abi.TF_SRGB)):
            for a, premult in ((None, False), (alpha, True)):
                got = rp.pngSamples(a, premultiplied=premult, bigEndian=True, **kw)
                exp = host.pngSamples(ctx, down, a, premultiplied=premult, bigEndian=True, **kw)
                assert np.array_equal(got, exp), "resident samples, orientation %d" % o
        assert_bits_equal(rp.download(), np.stack(down), "the planes are left as they were", any_nan=True)


def test_planes_taken_by_a_later_upload_are_an_error_not_other_pixels(ctx, resident_src):
    first = host.ResidentPlanes.upload(ctx, resident_src)
    second = host.ResidentPlanes.upload(ctx, resident_src[:, :5, :7])
    assert second.live() and not first.live()
    for call in (lambda: first.pngSamples(), lambda: first.colorPeak(), lambda: first.orient(3)):
        with pytest.raises(_lib.IllegalStateException):
            call()
    assert second.shape == (5, 7) and second.pngSamples().shape == (5, 7, 3)
    first.replace(resident_src)  # refilled: its own again
    assert first.live() and not second.live() and first.pngSamples().shape == (37, 53, 3)
