"""GPU, C ABI: the writers and the orientation on a device plane set -- jxl_canvas_png_samples, jxl_canvas_pfm_samples,
jxl_canvas_color_peak, jxl_canvas_orient -- against the stage entries (jxl_stage_png_samples, jxl_stage_pfm_samples,
jxl_stage_color_peak, jxl_stage_orient: existing code) on the planes downloaded from the set. Equality of bytes everywhere.

Sizes 5 x 7 (35 pixels: rows no multiple of 4, every lane group next to a scalar tail) and 33 x 130 (more than one workgroup)."""
import ctypes as C
import itertools

import numpy as np
import pytest

from conftest import assert_bits_equal
from jxlatte_amd import _lib, abi, host
from jxlatte_amd.decoder import PRI_BT2100, PRI_SRGB, WP_D65, get_conversion_matrix

pytestmark = pytest.mark.gpu
F = np.float32
SIZES = [(5, 7), (33, 130)]
MATRIX = get_conversion_matrix(PRI_BT2100, WP_D65, PRI_SRGB, WP_D65)
# the stage sets: an sRGB image written as it is (no stage changes a sample), and PQ samples through a gamut matrix and a peak scale to sRGB
STAGES = {"srgb identity": dict(tfIn=abi.TF_SRGB, tfOut=abi.TF_SRGB), "none": dict(),
          "pq + matrix": dict(tfIn=abi.TF_PQ, matrix=MATRIX, scale=F(1.37), tfOut=abi.TF_SRGB)}
# (alpha kind or None, premultiplied)
ALPHAS = [(None, False), ("int", False), ("float", False), ("int", True), ("float", True)]


def _colour(rng, shape, is_int):
    if is_int:
        a = rng.integers(0, 256, shape).astype(np.int32)
        a.flat[:6] = [0, 255, 256, -1, 2 ** 31 - 1, -2 ** 31]
    else:
        a = rng.uniform(-0.1, 1.2, shape).astype(F)
        a.flat[:8] = [0.0, -0.0, 1.0, np.nan, np.inf, -np.inf, 1e-45, 4.0]
    return a


def _alpha(rng, shape, kind):
    if kind == "int":
        a = rng.integers(0, 256, shape).astype(np.int32)
        a.flat[:5] = [0, 255, 300, -1, 1]
    else:
        a = rng.uniform(0, 1, shape).astype(F)
        a.flat[:7] = [0.0, -0.0, 1.0, 1.5, np.nan, np.inf, 1e-30]
    return a


def _set(ctx, shape, n_color, is_int, seed):
    """a set of n_color colour planes, an int32 alpha plane (index n_color) and a float one (n_color + 1)"""
    rng = np.random.default_rng(seed)
    arrays = [_colour(rng, shape, is_int) for _ in range(n_color)] + [_alpha(rng, shape, "int"), _alpha(rng, shape, "float")]
    return host.DeviceCanvas.fromArrays(ctx, arrays), arrays


@pytest.mark.parametrize("shape", SIZES)
@pytest.mark.parametrize("n_color,is_int", [(1, False), (1, True), (3, False), (3, True)])
def test_png_samples_of_a_set_equal_the_stage_entry(ctx, shape, n_color, is_int):
    cv, arrays = _set(ctx, shape, n_color, is_int, seed=shape[1] + n_color + is_int)
    try:
        src = [cv.download(i) for i in range(n_color)]
        n = 0
        for (sname, kw), depth, (akind, premult) in itertools.product(STAGES.items(), (8, 16), ALPHAS):
            kw = dict(kw, inMax=[255] * n_color) if is_int else kw
            ap = None if akind is None else n_color + (akind == "float")
            alpha = None if ap is None else cv.download(ap)
            common = dict(premultiplied=premult, bitDepth=depth, bigEndian=True, alphaDepth=8, colorDepth=8, **kw)
            exp = host.pngSamples(ctx, src, alpha, **common)
            ctx.blend_bus = [0, 0]
            got = cv.pngSamples(nColor=n_color, alphaPlane=ap, **common)
            what = "%s depth %d alpha %s premult %d" % (sname, depth, akind, premult)
            assert got.dtype == exp.dtype and got.shape == exp.shape, what
            assert np.array_equal(got, exp), what + ": %d samples differ" % int((got != exp).sum())
            assert ctx.blend_bus == [0, got.nbytes], what
            n += 1
        assert n == 3 * 2 * 5
    finally:
        cv.release()


@pytest.mark.parametrize("shape", SIZES)
def test_pfm_samples_and_peak_of_a_set_equal_the_stage_entries(ctx, shape):
    rng = np.random.default_rng(shape[0])
    for kinds in ([False], [True], [False] * 3, [True] * 3, [True, False, True]):
        arrays = [_colour(rng, shape, k) for k in kinds] + [_alpha(rng, shape, "float")]
        cv = host.DeviceCanvas.fromArrays(ctx, arrays)
        try:
            n = len(kinds)
            src = [cv.download(i) for i in range(n)]
            depths = [8, 16, 12][:n]
            assert np.array_equal(cv.pfmSamples(nColor=n, taggedDepths=depths), host.pfmSamples(ctx, src, depths)), kinds
            if len(set(kinds)) == 1:  # colorParams describes planes of one kind
                for kw in (dict(), dict(tfIn=abi.TF_SRGB), dict(tfIn=abi.TF_PQ, matrix=MATRIX)):
                    kw = dict(kw, inMax=[255] * n) if kinds[0] else kw
                    a, b = cv.colorPeak(nColor=n, **kw), host.determinePeak(ctx, src, **kw)
                    assert a.tobytes() == b.tobytes() or (np.isnan(a) and np.isnan(b)), (kinds, kw, a, b)
        finally:
            cv.release()


@pytest.mark.parametrize("shape", SIZES)
def test_orient_moves_every_plane_whatever_its_type(ctx, shape):
    rng = np.random.default_rng(shape[1])
    arrays = [_colour(rng, shape, False), _colour(rng, shape, True), _colour(rng, shape, False), _alpha(rng, shape, "int")]
    for orientation in range(1, 9):
        cv = host.DeviceCanvas.fromArrays(ctx, arrays)
        try:
            cv.orient(orientation)
            want = [host.transposeBuffer(ctx, a, orientation) for a in arrays]
            assert cv.shape == want[0].shape == ((shape[1], shape[0]) if orientation > 4 else shape)
            s = abi.CanvasShape()
            ctx.call("jxl_canvas_describe", cv.id, C.byref(s))
            assert (s.n, s.h, s.w) == (4,) + cv.shape and list(s.types)[:4] == cv.types
            for i, a in enumerate(want):
                assert_bits_equal(cv.download(i), a, "orientation %d plane %d" % (orientation, i), any_nan=False)
            # the writers read the set as it stands now
            assert np.array_equal(cv.pfmSamples(nColor=3, taggedDepths=[8, 8, 8]), host.pfmSamples(ctx, want[:3], [8, 8, 8]))
        finally:
            cv.release()
    cv = host.DeviceCanvas.fromArrays(ctx, arrays)
    try:
        for bad in (0, 9, -1):
            with pytest.raises(_lib.IllegalStateException):
                cv.orient(bad)
        assert cv.shape == shape
    finally:
        cv.release()


def _png_call(ctx, id_, alpha_plane, p, out):
    return ctx.lib.jxl_canvas_png_samples(ctx.h, id_, alpha_plane, C.byref(p) if p is not None else None, out.ctypes.data if out is not None else None)


def test_mismatched_parameters_are_refused_with_out_untouched(ctx):
    shape = (5, 7)
    cv, arrays = _set(ctx, shape, 3, False, seed=1)  # float colours, int32 alpha at 3, float alpha at 4
    INV = abi.JXL_ERR_INVALID_ARGUMENT
    fl = [np.zeros(shape, F)] * 3
    it = [np.zeros(shape, np.int32)] * 3
    ai, af = np.zeros(shape, np.int32), np.zeros(shape, F)
    try:
        def png(p, alpha_plane, id_=None):
            out = np.full(5 * 7 * 4 * 2 + 16, 0xA5, np.uint8)
            st = _png_call(ctx, cv.id if id_ is None else id_, alpha_plane, p, out)
            assert np.all(out == 0xA5), "out was written"
            return st

        good = host.pngParams(fl, shape, alpha=ai, bitDepth=8)
        out = np.full(5 * 7 * 4 + 16, 0xA5, np.uint8)
        assert _png_call(ctx, cv.id, 3, good, out) == abi.JXL_OK and np.all(out[5 * 7 * 4:] == 0xA5) and not np.all(out[:5 * 7 * 4] == 0xA5)
        assert png(host.pngParams(it, shape, alpha=ai, bitDepth=8, inMax=[255] * 3), 3) == INV      # colour tag
        assert png(host.pngParams(fl, shape, alpha=af, bitDepth=8), 3) == INV                        # alpha tag (plane 3 is int32)
        assert png(host.pngParams(fl, shape, alpha=ai, bitDepth=8), 4) == INV                        # alpha tag (plane 4 is float)
        assert png(host.pngParams(fl, (7, 5), alpha=ai, bitDepth=8), 3) == INV                       # the set's size
        assert png(host.pngParams(fl, (5, 8), alpha=ai, bitDepth=8), 3) == INV
        assert png(host.pngParams(fl, shape, alpha=ai, bitDepth=8), -1) == INV                       # has_alpha without a plane
        assert png(host.pngParams(fl, shape, bitDepth=8), 3) == INV                                  # a plane without has_alpha
        assert png(good, 5) == INV and png(good, -2) == INV                                          # no such plane
        assert png(good, 3, id_=cv.id + 100) == INV and png(good, 3, id_=-1) == INV                  # no such set
        assert png(None, 3) == INV
        assert _png_call(ctx, cv.id, 3, good, None) == INV
        # what jxl_stage_png_samples refuses
        assert png(host.pngParams(fl, shape, alpha=ai, bitDepth=12), 3) == INV
        assert png(host.pngParams(fl, shape, alpha=ai, bitDepth=8, maxValue=255), 3) == INV
        assert png(host.pngParams(fl, shape, alpha=ai, bitDepth=8, alphaDepth=0, premultiplied=True), 3) == INV
        assert png(host.pngParams(fl, shape, alpha=ai, bitDepth=8, tfIn=9), 3) == INV
        assert png(host.pngParams(fl, shape, alpha=ai, bitDepth=8, tfIn=abi.TF_HLG), 3) == abi.JXL_ERR_UNSUPPORTED
        p = host.pngParams(fl, shape, alpha=ai, bitDepth=8)
        p.color.n_planes = 2
        assert png(p, 3) == INV

        def pfm(p, id_=None):
            out = np.full(5 * 7 * 3 * 4 + 16, 0xA5, np.uint8)
            st = ctx.lib.jxl_canvas_pfm_samples(ctx.h, cv.id if id_ is None else id_, C.byref(p), out.ctypes.data)
            assert np.all(out == 0xA5), "out was written"
            return st

        assert pfm(host.pfmParams([it[0], fl[1], fl[2]], shape, [8, 8, 8])) == INV                   # plane 0 is float
        assert pfm(host.pfmParams(fl, (7, 5))) == INV
        assert pfm(host.pfmParams(fl, shape), id_=77) == INV
        p = host.pfmParams(fl, shape)
        p.n_planes = 2
        assert pfm(p) == INV
        assert ctx.lib.jxl_canvas_pfm_samples(ctx.h, cv.id, C.byref(host.pfmParams(fl, shape)), None) == INV
        peak = C.c_float(-3.0)
        assert ctx.lib.jxl_canvas_color_peak(ctx.h, cv.id, C.byref(host.colorParams(it, inMax=[255] * 3)), C.byref(peak)) == INV
        assert ctx.lib.jxl_canvas_color_peak(ctx.h, 55, C.byref(host.colorParams(fl)), C.byref(peak)) == INV
        assert peak.value == -3.0
    finally:
        cv.release()
    # a grey set has no three colour planes
    g = host.DeviceCanvas.fromArrays(ctx, [np.zeros(shape, F)])
    try:
        out = np.full(5 * 7 * 3 + 16, 0xA5, np.uint8)
        assert _png_call(ctx, g.id, -1, host.pngParams(fl, shape, bitDepth=8), out) == INV and np.all(out == 0xA5)
    finally:
        g.release()
