"""GPU, stage level: the entry points a Modular frame's restoration and colour stages reach -- host.performGabConvolution,
host.performEdgePreservingFilter(..., None, invModularSigma) with the CONSTANT inverse sigma, the one-colour forms of both,
host.modularToFloat with two inputs (the wrapping sum included), invertXYB and performColorTransformsYCbCr -- through the device
backend's hooks, against the float64 models (vardct_ref64, pixel_ref64) on the shapes and sigmas of tests/jxl_writer_lossy_cases.py:
planes that are NOT padded to 8, down to 1 x 1 where mirrorCoordinate reflects more than once, up to 70 which crosses the
restoration kernels' workgroups. No oracle in any assertion.

K: the stage rows of test_vardct_ref64_cpu.K_STAGE (Gaborish 12, EPF 36, XYB 4) and test_pixel_ref64_cpu.K["to_float"]. The YCbCr
loop has no row there; K_YCBCR = 5 is derived: the longest chain of a sample is Y + offset, two products and two sums
(JXLCodestreamDecoder.java:275-279), five roundings of partial results that the companion bounds, the float constants taken as exact."""
import numpy as np
import pytest

import jxl_writer_lossy_cases as C
import pixel_ref64 as P
import vardct_ref64 as M
from test_device_frames_gpu import CountingBackend
from test_pixel_ref64_cpu import K
from test_vardct_ref64_cpu import K_STAGE

pytestmark = pytest.mark.gpu
F = np.float32
K_YCBCR = 5
SIGMAS = (1.0, 1.5, 2.0, 0.25)
RF = dict(channel_scale=[40.0, 5.0, 3.5], pass0=float(F(0.9)), pass2=6.5, border_sad_mul=float(F(2) / F(3)))
RF_CUSTOM = dict(channel_scale=[30.0, 7.0, 2.5], pass0=0.75, pass2=5.0, border_sad_mul=0.5)
GAB_DEFAULT = ([float(F(0.115169525))] * 3, [float(F(0.061248592))] * 3)
GAB_CUSTOM = ([0.115, 0.2, 0.05], [0.061, 0.01, 0.1])
_planes = {}


@pytest.fixture(scope="module")
def backend(ctx):
    return CountingBackend(ctx)


def xyb_space(h, w):
    """float32 planes X, Y, B of a frame of jxl_writer_lossy_cases' kind: the stream's integers through the model of modularToFloat"""
    if (h, w) not in _planes:
        y, x, b = C.xyb_planes(np.random.default_rng(7600 + 100 * h + w), h, w)
        lfd = [F(1.0 / 4096.0), F(1.0 / 512.0), F(1.0 / 256.0)]
        _planes[h, w] = np.stack([P.modular_to_float(x, None, lfd[0])[0], P.modular_to_float(y, None, lfd[1])[0],
                                  P.modular_to_float(y, b, lfd[2])[0]]).astype(F)
    return _planes[h, w]


def one_colour(h, w):
    p = C.int_planes(np.random.default_rng(7700 + 100 * h + w), h, w, 8, 1)[0]
    return (p.astype(F) * (F(1) / F(255)))[None].astype(F)


def hold(got, model, what, k):
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == model[0].shape, what
    r = M.error_ratio(got, *model)
    print("%s: ratio %.3f of K = %d" % (what, r, k))
    assert r <= k, (what, r, k)
    return r


def epf_args(rf):
    return rf["channel_scale"], rf["pass0"], rf["pass2"], rf["border_sad_mul"]


@pytest.mark.parametrize("size", C.SIZES, ids=lambda s: "%dx%d" % s)
def test_gaborish_on_planes_of_any_size(backend, size):
    p = xyb_space(*size)
    for name, (w1, w2) in (("default", GAB_DEFAULT), ("custom", GAB_CUSTOM)):
        hold(backend.gab(p, w1, w2), M.gab(p, np.abs(p), w1, w2), "gab %dx%d %s weights" % (*size, name), K_STAGE["gab"])
    g = one_colour(*size)
    w1, w2 = GAB_CUSTOM
    x, a = M.gab(np.repeat(g, 3, 0), np.abs(np.repeat(g, 3, 0)), [w1[0]] * 3, [w2[0]] * 3)
    hold(backend.gab(g, w1, w2), (x[:1], a[:1]), "gab %dx%d one colour" % size, K_STAGE["gab"])


@pytest.mark.parametrize("iters", (1, 2, 3))
@pytest.mark.parametrize("size", C.SIZES, ids=lambda s: "%dx%d" % s)
def test_epf_with_the_constant_sigma(backend, size, iters):
    """three colours and one, every sigma of the cases: 1.0, 1.5 and 2.0 filter, 0.25 copies (its inverse 4 > 1 / 0.3)"""
    p, g = xyb_space(*size), one_colour(*size)
    g3 = np.repeat(g, 3, 0)
    for sigma in SIGMAS:
        inv = float(F(F(1) / F(sigma)))
        for name, rf in (("default", RF), ("custom", RF_CUSTOM)):
            what = "%dx%d it%d sigma %g %s fields" % (*size, iters, sigma, name)
            x, a = M.epf(p, np.abs(p), iters, inv, *epf_args(rf))
            got = backend.epf(p, iters, None, inv, rf)
            hold(got, (x, a), "epf " + what, K_STAGE["epf"])
            x1, a1 = M.epf(g3, np.abs(g3), iters, inv, *epf_args(rf))
            got1 = backend.epf(g, iters, None, inv, rf)
            hold(got1, (x1[:1], a1[:1]), "epf one colour " + what, K_STAGE["epf"])
            if sigma == 0.25:  # copied: bit for bit the input
                assert np.array_equal(got.view(np.uint32), p.view(np.uint32)) and np.array_equal(got1.view(np.uint32), g.view(np.uint32)), what
            elif min(size) > 1:
                assert (got != p).mean() > 0.2, what  # and the filter ran


def test_the_models_tell_a_wrong_filter(backend):
    """the comparisons discriminate: sigma in place of 1 / sigma, the one-colour distance counted once, planes padded to 8"""
    p, g = xyb_space(13, 21), one_colour(13, 21)
    got = backend.epf(p, 2, None, 0.5, RF)
    assert M.error_ratio(got, *M.epf(p, np.abs(p), 2, 2.0, *epf_args(RF))) > 100 * K_STAGE["epf"]
    got = backend.epf(g, 2, None, 1.0, RF)
    g3 = np.repeat(g, 3, 0)
    x, a = M.epf(g3, np.abs(g3), 2, 1.0, [40.0, 0.0, 0.0], *epf_args(RF)[1:])
    assert M.error_ratio(got, x[:1], a[:1]) > 100 * K_STAGE["epf"]
    pad = np.pad(p, ((0, 0), (0, 3), (0, 3)))
    x, a = M.gab(pad, np.abs(pad), *GAB_DEFAULT)
    assert M.error_ratio(backend.gab(p, *GAB_DEFAULT), x[:, :13, :21], a[:, :13, :21]) > 100 * K_STAGE["gab"]


@pytest.mark.parametrize("size", C.SIZES + ((9, 11),), ids=lambda s: "%dx%d" % s)
def test_modular_to_float_with_two_inputs(backend, size):
    """scale * (a + b) with Java's wrapping int sum (Frame.java:441): small values and values whose sum leaves int32 both ways"""
    rng = np.random.default_rng(7800 + size[0])
    a = rng.integers(-(1 << 31), 1 << 31, size).astype(np.int64)
    b = rng.integers(-(1 << 31), 1 << 31, size).astype(np.int64)
    a.reshape(-1)[:1], b.reshape(-1)[:1] = (1 << 31) - 1, 1
    if a.size > 4:
        a.reshape(-1)[1:4], b.reshape(-1)[1:4] = ((1 << 31) - 1, -(1 << 31), -(1 << 31)), ((1 << 31) - 1, -1, -(1 << 31))
        assert (a + b >= 1 << 31).any() and (a + b < -(1 << 31)).any()
    y, _, bmy = C.xyb_planes(rng, *size)
    for scale in (1.0 / 256.0, float(F(0.75) * F(1.0 / 128.0))):
        for u, v, what in ((a, b, "wrapping"), (y, bmy, "Y + (B - Y)")):
            got = backend.modular_to_float(u.astype(np.int32), v.astype(np.int32), scale)
            hold(got, P.modular_to_float(u, v, scale), "modularToFloat %dx%d %s x %g" % (*size, what, scale), K["to_float"])
            hold(backend.modular_to_float(u.astype(np.int32), None, scale), P.modular_to_float(u, None, scale),
                 "modularToFloat %dx%d one input x %g" % (*size, scale), K["to_float"])


@pytest.mark.parametrize("size", C.SIZES, ids=lambda s: "%dx%d" % s)
def test_colour_transforms(backend, size):
    p = xyb_space(*size)
    bias = [F(C.OPSIN_BIAS)] * 3
    cbrt = [F(np.cbrt(np.float64(b))) for b in bias]
    matrix = [F(v) for v in C.DEFAULT_OPSIN]
    for target in (255.0, 1000.0):
        hold(backend.xyb(p, matrix, bias, cbrt, target), M.xyb(p, np.abs(p), matrix, bias, cbrt, target), "xyb %dx%d target %g" % (*size, target),
             K_STAGE["xyb"])
    rng = np.random.default_rng(7900 + size[0])
    ycc = np.stack([q.astype(F) * (F(1) / F(255)) for q in C.int_planes(rng, *size, 8, 3, centred=(0, 2))]).astype(F)
    x, a = M.ycbcr(ycc, np.abs(ycc))
    hold(backend.ycbcr(ycc), (x, a), "ycbcr %dx%d" % size, K_YCBCR)
    assert M.error_ratio(backend.ycbcr(ycc), *M.ycbcr(ycc[::-1], np.abs(ycc[::-1]))) > 100 * K_YCBCR
