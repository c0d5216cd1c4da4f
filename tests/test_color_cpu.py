"""CPU-only ground for the device colour management (csrc/k_color.hip): the accuracy of the header's pow (numpy restatement of
tests/test_fastpow_cpu.py) for the exponents of the new curves, the 1-ulp bound of every new transfer direction with that
pow in place of Math.pow, the decisions JXLImage.transform(device=True) takes, the bindings and the command line."""
import ctypes as C
import os
import types

import numpy as np
import pytest

import color_ref as ref
from test_fastpow_cpu import fast_pow
from jxlatte_amd import abi, decoder, host
from jxlatte_amd.decoder import (CE_GRAY, CE_RGB, PEAK_DETECT_AUTO, PEAK_DETECT_OFF, PEAK_DETECT_ON, PRI_BT2100, PRI_P3, PRI_SRGB,
                                 TF_BT709, TF_DCI, TF_HLG, TF_LINEAR, TF_PQ, TF_SRGB, WP_D65, JXLImage, UnsupportedOperationException)

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the exponents of the curves k_color.hip evaluates through fp_pow: sRGB, BT.709 (both ways), PQ to linear (two), DCI and gamma 2.2
EXPONENTS = [2.4, 2.2222222222222222222, 0.45, 0.012683313515655965121, 6.2725880551301684533, 2.6, 1 / 2.6, 2.2, 1 / 2.2, 1e7 / 3846154, 1e-7 * 3846154,
             1e7 / 4545455, 1e-7 * 4545455, 1e7 / 5555556, 1e-7 * 5555556]


def _bases():
    rng = np.random.default_rng(11)
    f = np.concatenate([rng.uniform(0, 1, 150000), rng.uniform(1, 4, 50000), 10 ** rng.uniform(-45, 4, 100000),
                        10 ** rng.uniform(-12, 0, 50000)]).astype(F)
    return f[f > 0].astype(np.float64)


@pytest.mark.parametrize("p", EXPONENTS)
def test_fast_pow_relative_error_for_the_new_exponents(p):
    """the 1-ulp float bound of the double-pow curves rests on a relative error near 1e-13 wherever the result is a float
    (normal or denormal): measured against 80-bit long double over float bases from the smallest denormal to 1e4"""
    x = _bases()
    with np.errstate(over="ignore", under="ignore"):
        exact = np.power(x.astype(np.longdouble), np.longdouble(p))
        got = fast_pow(x, p)
    ok = (exact > np.longdouble(1e-46)) & (exact < np.longdouble(3.5e38))
    rel = np.abs((got[ok].astype(np.longdouble) - exact[ok]) / exact[ok])
    print("p = %.17g: max relative error %.3g over %d bases" % (p, float(rel.max()), int(ok.sum())))
    assert float(rel.max()) < 1e-13, (p, float(rel.max()))


def _fp_pow(x, p):
    """fp_pow of csrc/jxl_fastpow.h: the series for finite positive bases, Math.pow's special results elsewhere"""
    x = np.asarray(x, np.float64)
    pos = (x > 0) & np.isfinite(x)
    with np.errstate(all="ignore"):
        r = np.where(pos, fast_pow(np.where(pos, x, 1.0), p), np.where(x == 0, 0.0, np.where(np.isinf(x), np.inf, np.nan)))
    return r


def _samples(n):
    rng = np.random.default_rng(12)
    return np.concatenate([rng.uniform(0, 1, n), rng.uniform(1, 4, n // 8), 10 ** rng.uniform(-12, 0, n // 8),
                           rng.integers(1, 1 << 23, n // 8).astype(np.uint32).view(F).astype(np.float64),
                           [0.0, -0.0, -1e-3, -2.0, np.inf, -np.inf, np.nan]]).astype(F)


DIRECTIONS = [("to", "srgb", 0), ("to", "bt709", 0), ("to", "pq", 0), ("to", "gamma", 3846154), ("to", "gamma", 4545455),
              ("to", "gamma", 5555556), ("from", "bt709", 0), ("from", "gamma", 3846154), ("from", "gamma", 4545455),
              ("from", "gamma", 5555556)]


@pytest.mark.parametrize("way,tf,gamma", DIRECTIONS)
def test_curves_with_the_header_pow_are_within_one_ulp_of_libm(way, tf, gamma):
    """every new transfer direction, restated once with math.pow and once with the header's pow: at most 1 float ulp apart, the
    same NaNs, zeros and infinities, identical on the linear segments"""
    f = _samples(120000)
    fn = ref.to_linear if way == "to" else ref.from_linear
    a, lin = fn(tf, f, gamma)
    b, _ = fn(tf, f, gamma, jpow=_fp_pow)
    special = np.isnan(a) | np.isnan(b) | (a == 0) | (b == 0) | np.isinf(a) | np.isinf(b)
    assert np.array_equal(np.isnan(a), np.isnan(b))
    assert np.array_equal(a[special & ~np.isnan(a)], b[special & ~np.isnan(a)])
    assert np.array_equal(a[lin].view(np.uint32), b[lin].view(np.uint32))
    d = ref.ulp_distance(a[~special], b[~special])
    print("%s %s %d: %.4f %% identical" % (way, tf, gamma, 100.0 * float((d == 0).mean())))
    assert int(d.max()) <= 1


def test_pq_to_linear_is_nan_below_its_boundary():
    """TransferFunction.java:89-92: pow(f, 0.0127) below 0.8359375 makes the base of the second pow negative"""
    v, _ = ref.to_linear("pq", np.array([0.0, 1e-7, 7.0e-7, 7.6e-7, 0.5], F))
    assert np.isnan(v[:3]).all() and np.isfinite(v[3:]).all()


def test_color_params_layout_and_selectors():
    assert C.sizeof(abi.ColorParams) == 4 * (2 + 3 + 2 + 2 + 1 + 9 + 3)
    hdr = open(os.path.join(ROOT, "include", "jxlatte_amd.h")).read()
    for name in ("LINEAR", "SRGB", "BT709", "PQ", "GAMMA", "HLG"):
        assert "#define JXL_TF_%-6s %d" % (name, getattr(abi, "TF_" + name)) in hdr
    assert decoder._tf_selector(TF_DCI) == (abi.TF_GAMMA, 3846154)
    assert decoder._tf_selector(4545455) == (abi.TF_GAMMA, 4545455)
    assert decoder._tf_selector(TF_BT709) == (abi.TF_BT709, 0)
    with pytest.raises(UnsupportedOperationException):
        decoder._tf_selector(TF_HLG)
    with pytest.raises(ValueError):
        decoder._tf_selector((1 << 24) + 3)
    p = host.colorParams([np.zeros((2, 2), np.int32)] * 3, tfIn=abi.TF_PQ, inMax=[255, 255, 255], scale=2.0, matrix=np.eye(3), maxValue=255)
    assert (p.n_planes, p.in_is_int, list(p.in_max), p.use_scale, p.scale, p.use_matrix, p.matrix[4], p.max_value) == (3, 1, [255] * 3, 1, 2.0, 1, 1.0, 255)
    with pytest.raises(ValueError):
        host.colorParams([np.zeros((2, 2), np.int32), np.zeros((2, 2), F), np.zeros((2, 2), F)])


def _info(gray=False, bits=8, transfer=TF_SRGB, prim=PRI_SRGB, xyb=False):
    return types.SimpleNamespace(colour_space=CE_GRAY if gray else CE_RGB, num_extra=0, ec_type=[], ec_alpha_associated=[], ec_bits=[],
                                 prim_xy=list(prim), white_xy=list(WP_D65), transfer=transfer, xyb_encoded=xyb,
                                 bits_per_sample=bits, use_icc=False)


class _Recorder:
    """a backend that has color_convert: records the calls, answers with planes of the right count"""

    def __init__(self, peak):
        self.calls, self.peak = [], F(peak)

    def color_peak(self, planes, **kw):
        self.calls.append(("peak", len(planes), kw))
        return self.peak

    def color_convert(self, planes, **kw):
        self.calls.append(("convert", len(planes), kw))
        n = 3 if (len(planes) == 3 or kw.get("matrix") is not None) else 1
        return [np.zeros(planes[0].shape, F) for _ in range(n)]

    def transfer(self, plane, tf):  # the host path's one device stage
        return np.zeros(plane.shape, F)


def _meta(im):
    return (im.transfer_, [float(v) for v in im.primariesXY], [float(v) for v in im.whiteXY], im.colorEncoding, list(im.bitDepths),
            len(im.buffer), [b.dtype for b in im.buffer], [b.shape for b in im.buffer])


def test_device_transform_takes_the_references_decisions():
    rng = np.random.default_rng(3)
    ints = [rng.integers(0, 256, (4, 5)).astype(np.int32) for _ in range(3)]
    flts = [rng.random((4, 5)).astype(F) for _ in range(3)]
    # P3 int8 -> sRGB: linearize is the first stage (max 255), a matrix, no peak
    be = _Recorder(0.5)
    im = JXLImage(ints, _info(prim=PRI_P3), be)
    out = im.transform(PRI_SRGB, WP_D65, TF_SRGB, PEAK_DETECT_AUTO, device=True)
    (kind, n, kw), = be.calls
    assert kind == "convert" and n == 3 and kw["inMax"] == [255] * 3 and kw["scale"] is None and kw["tfIn"] == abi.TF_SRGB and kw["tfOut"] == abi.TF_SRGB
    assert np.array_equal(kw["matrix"], decoder.get_conversion_matrix(PRI_SRGB, WP_D65, PRI_P3, WP_D65))
    assert _meta(out) == _meta(im.transform(PRI_SRGB, WP_D65, TF_SRGB, PEAK_DETECT_AUTO))
    # same primaries, same transfer: the image itself, no call
    be.calls.clear()
    assert im.transform(PRI_P3, WP_D65, TF_SRGB, device=True) is im and not be.calls
    # linear int image -> sRGB, same primaries: transferInPlace casts with the depth itself (JXLImage.java:248)
    im = JXLImage(ints, _info(transfer=TF_LINEAR), be)
    im.transform(PRI_SRGB, WP_D65, TF_SRGB, device=True)
    assert be.calls[-1][2]["inMax"] == [8] * 3 and "matrix" not in be.calls[-1][2]
    # PQ BT.2100 float -> sRGB: one peak over the tone-mapped image, then the scale (peak 0.5 -> 2)
    be.calls.clear()
    im = JXLImage(flts, _info(transfer=TF_PQ, prim=PRI_BT2100, bits=16), be)
    out = im.transform(PRI_SRGB, WP_D65, TF_SRGB, PEAK_DETECT_AUTO, device=True)
    assert [c[0] for c in be.calls] == ["peak", "convert"] and be.calls[0][2].get("matrix") is not None
    assert be.calls[1][2]["scale"] == F(2.0)
    assert _meta(out) == _meta(im.transform(PRI_SRGB, WP_D65, TF_SRGB, PEAK_DETECT_AUTO))
    for peak, pd, scaled, asked in ((2.0, PEAK_DETECT_AUTO, False, True), (2.0, PEAK_DETECT_ON, True, True), (0.5, PEAK_DETECT_OFF, False, False),
                                    (float("nan"), PEAK_DETECT_AUTO, False, True)):
        be = _Recorder(peak)
        im = JXLImage(flts, _info(transfer=TF_PQ, prim=PRI_BT2100, bits=16), be)
        im.transform(PRI_SRGB, WP_D65, TF_SRGB, pd, device=True)
        assert ([c[0] for c in be.calls] == ["peak", "convert"]) == asked and (be.calls[-1][2]["scale"] is not None) == scaled
    # to PQ or linear: no peak; a linear target after the matrix skips transfer() altogether
    be = _Recorder(0.5)
    im = JXLImage(flts, _info(transfer=TF_PQ, prim=PRI_BT2100, bits=16), be)
    out = im.transform(PRI_SRGB, WP_D65, TF_LINEAR, device=True)
    assert [c[0] for c in be.calls] == ["convert"] and "tfOut" not in be.calls[0][2]
    assert _meta(out) == _meta(im.transform(PRI_SRGB, WP_D65, TF_LINEAR))
    # grey, gamma-tagged, 16 bit, other primaries: three planes come back and the image becomes RGB
    be = _Recorder(0.5)
    g = [rng.integers(0, 65536, (4, 5)).astype(np.int32)]
    im = JXLImage(g, _info(gray=True, bits=16, transfer=4545455, prim=PRI_P3), be)
    out = im.transform(PRI_SRGB, WP_D65, TF_SRGB, device=True)
    assert be.calls[-1][1] == 1 and be.calls[-1][2]["gammaIn"] == 4545455 and be.calls[-1][2]["inMax"] == [65535]
    assert _meta(out) == _meta(im.transform(PRI_SRGB, WP_D65, TF_SRGB))
    assert out.colorEncoding == CE_RGB and len(out.buffer) == 3 and out.bitDepths == [16, 16, 16]


def test_host_path_still_refuses_bt709_dci_and_gamma_targets():
    flts = [np.full((2, 3), 0.5, F) for _ in range(3)]
    for be in (_Recorder(1.0), types.SimpleNamespace(transfer=lambda plane, tf: plane)):  # the second has no color_convert
        im = JXLImage(flts, _info(transfer=TF_LINEAR), be)
        for target in (TF_BT709, TF_DCI, 4545455):
            with pytest.raises(UnsupportedOperationException):
                im.transform(PRI_SRGB, WP_D65, target)  # device=False: as before
        if not hasattr(be, "color_convert"):
            with pytest.raises(UnsupportedOperationException):
                im.transform(PRI_SRGB, WP_D65, TF_BT709, device=True)  # no device entry in this backend: the host path
        else:
            assert im.transform(PRI_SRGB, WP_D65, TF_BT709, device=True).transfer_ == TF_BT709


def test_cli_switches_parse():
    from jxlatte_amd.__main__ import main
    sample = os.path.join(ROOT, "tests", "golden", "samples", "lenna.jxl")
    assert main([sample, "--info", "--device-color", "--png-peak-detect=on"]) == 0
    assert main([sample, "--info", "--png-peak-detect", "off"]) == 0
    with pytest.raises(SystemExit):
        main([sample, "--info", "--png-peak-detect=sometimes"])


def test_reference_peak_restatement():
    nan = F("nan")
    assert ref.row_max([F(3), F(1), nan, F(2)]) == 1 and np.isnan(ref.row_max([nan, F(1)]))
    assert np.signbit(ref.row_max([F(-0.0), F(0.0)])) and not np.signbit(ref.row_max([F(0.0), F(-0.0)]))
    assert np.isnan(ref.determine_peak(np.array([[1, 2], [nan, 0]], F)))
    assert np.signbit(ref.determine_peak(np.array([[-0.0, 5]], F))) and not np.signbit(ref.determine_peak(np.array([[-0.0, 5], [0.0, 1]], F)))
    assert ref.determine_peak(np.array([[3, 200], [7, 1]], np.int32), 255) == F(200) / F(255)
