"""HDR -> SDR tone mapping on the device (jxl_ctx_set_tone_map; csrc/tone_map_ops.h inside every colour pass).

  * the float exits against the float64 model of tests/tone_map_model.py, held to 4 x the distance of the model's float32
    restatement from it, measured here per output curve and printed (profiles/tone_map.md has the values);
  * the identity setting gives the bytes of the same call without tone mapping;
  * one operator everywhere: the integer exits, the resized and the batched exits equal existing entries applied to the device's
    own tone-mapped float planes, bit for bit;
  * arming leaves nothing behind; the peak and PFM entries ignore it; a scale is refused while armed.
Sizes: 8 x 8, 67 x 83 (ragged; an odd plane size for the element-wise stores) and 264 x 40 (more than one workgroup row)."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import resize_ref as rr
import tone_map_model as tm
from jxlatte_amd import _lib, abi, host
from jxlatte_amd.decoder import (CE_GRAY, CE_RGB, PEAK_DETECT_OFF, PRI_BT2100, PRI_SRGB, TF_LINEAR, TF_PQ, TF_SRGB, WP_D65, DeviceBackend, JXLImage,
                                 PNGWriter, ToneMap, _primaries_to_xyz, toTensorBatch)

pytestmark = pytest.mark.gpu
F = np.float32
SHAPES = [(8, 8), (67, 83), (264, 40)]
UNIT, SOURCE, TARGET = 10000.0, 1000.0, 203.0
LUM = [float(x) for x in _primaries_to_xyz(PRI_BT2100, WP_D65)[1]]  # the weights the library is handed for BT.2020 samples
CURVES = {"linear": abi.TF_LINEAR, "srgb": abi.TF_SRGB, "bt709": abi.TF_BT709}


class armed:
    """the session's context tone-maps inside this block, and never after it"""

    def __init__(self, ctx, unit=UNIT, source=SOURCE, target=TARGET, gamut=True, lum=LUM):
        self.ctx, self.p = ctx, host.toneMapParams(lum, unit, source, target, gamut)

    def __enter__(self):
        host.setToneMap(self.ctx, self.p)

    def __exit__(self, *exc):
        host.setToneMap(self.ctx, None)
        return False


@pytest.fixture(scope="module")
def data():
    """the inputs of every test here, made once and never written"""
    d = {s: tm.pixels(s[0], s[1], seed, UNIT, SOURCE, TARGET, LUM) for seed, s in enumerate(SHAPES, 1)}
    rng = np.random.default_rng(9)
    d["pq16"] = [rng.integers(0, 65536, (67, 83)).astype(np.int32) for _ in range(3)]  # 16-bit PQ code values: up to 10000 nits
    d["grey"] = [np.ascontiguousarray(d[(67, 83)][1])]
    for v in d.values():
        for a in v:
            a.setflags(write=False)
    return d


def _bound_and_model(v, gamut, curve, lum=LUM):
    exact = [tm.curve64(p, curve) for p in tm.model(v, lum, UNIT, SOURCE, TARGET, gamut)]
    rest = [tm.curve32(p, curve) for p in tm.restated(v, lum, UNIT, SOURCE, TARGET, gamut)]
    bound = 0.0
    for r, e in zip(rest, exact):
        ok = np.isfinite(e)
        bound = max(bound, float(np.max(np.abs(r.astype(np.float64)[ok] - e[ok]))))
    return bound, exact


def _close(got, exact, bound, what):
    worst = 0.0
    for g, e in zip(got, exact):
        assert g.dtype == np.float32 and np.array_equal(np.isnan(g), np.isnan(e)), what + ": NaN maps to NaN, and nothing else does"
        ok = np.isfinite(e)
        worst = max(worst, float(np.max(np.abs(g.astype(np.float64)[ok] - e[ok]))))
    print("%s: device |err| %.3e, witness bound %.3e (held to 4 x)" % (what, worst, bound))
    assert worst <= 4 * bound, (what, worst, bound)


def _tensor(ctx, planes, dtype="float32", layout="CHW", channels=3, **kw):
    """host.tensorSamples into 0xA5-filled torch memory: the elements as numpy, [C][H][W] or [H][W][C]"""
    shape = planes[0].shape
    t = {"float32": torch.float32, "uint8": torch.uint8}[dtype]
    out = torch.empty((channels,) + shape if layout == "CHW" else shape + (channels,), dtype=t, device="cuda:%d" % ctx.device)
    out.view(torch.uint8).fill_(0xA5)
    host.tensorSamples(ctx, planes, None, out.data_ptr(), dtype=dtype, layout=layout, **kw)
    return out.cpu().numpy()


def _resized(ctx, call, size, channels=3, dtype=torch.float32, n=1):
    out = torch.empty((n, channels) + tuple(size), dtype=dtype, device="cuda:%d" % ctx.device)
    out.view(torch.uint8).fill_(0xA5)
    call(out.data_ptr())
    return out.cpu().numpy()


def _backend(ctx):
    """a DeviceBackend over the session's context"""
    be = DeviceBackend.__new__(DeviceBackend)
    be.host, be.ctx, be.palette_log = host, ctx, []
    return be


def _info(gray=False, transfer=TF_LINEAR, bits=16, intensity=SOURCE):
    return types.SimpleNamespace(colour_space=CE_GRAY if gray else CE_RGB, num_extra=0, ec_type=[], ec_alpha_associated=[], ec_bits=[],
                                 prim_xy=list(PRI_BT2100), white_xy=list(WP_D65), transfer=transfer, xyb_encoded=False, bits_per_sample=bits,
                                 use_icc=False, intensity_target=intensity)


TONE = ToneMap(TARGET, sourceNits=SOURCE, unitNits=UNIT)


# ---- the float exits against the float64 model ----
@pytest.mark.parametrize("shape", SHAPES)
def test_float_exits_against_the_model(ctx, data, shape):
    v = data[shape]
    for gamut in (False, True):
        for curve, tf in CURVES.items():
            bound, exact = _bound_and_model(v, gamut, curve)
            what = "%dx%d gamut %d %s" % (shape[0], shape[1], gamut, curve)
            with armed(ctx, gamut=gamut):
                got = host.colorConvert(ctx, v, tfOut=tf)
                ten = _tensor(ctx, v, tfOut=tf)
            _close(got, exact, bound, what + " color_convert")
            assert all(np.array_equal(ten[c].view(np.uint32), got[c].view(np.uint32)) for c in range(3)), what + ": the float32 tensor is the same operator"
    # where the luminance is not positive the pixel is v * norm, exactly (the gamut step off, a linear output)
    with armed(ctx, gamut=False):
        got = host.colorConvert(ctx, v)
    y = ((F(LUM[0]) * v[0]).astype(F) + (F(LUM[1]) * v[1]).astype(F)).astype(F) + (F(LUM[2]) * v[2]).astype(F)
    flat = ~(y > 0)
    assert flat.sum() >= 3  # the zero, the all-negative and the NaN pixel
    for g, a in zip(got, v):
        assert np.array_equal(g[flat], (a * F(UNIT / TARGET)).astype(F)[flat], equal_nan=True)


def test_transform_on_the_device_against_the_model(ctx, data):
    v = data[(67, 83)]
    im = JXLImage([a.copy() for a in v], _info(), _backend(ctx))
    res = im.transform(PRI_BT2100, WP_D65, TF_SRGB, device=True, toneMap=TONE)
    bound, exact = _bound_and_model(v, True, "srgb")
    _close(res.buffer[:3], exact, bound, "transform(device=True) srgb")
    assert not ctx.toneMapArmed() and res.transfer_ == TF_SRGB


def test_pq_tagged_integers_and_a_grey_image(ctx, data):
    # 16-bit PQ code values: the cast and the reference's PQ curve are the pinned entry's; the operator then meets the model on them
    pq = data["pq16"]
    lin = host.colorConvert(ctx, pq, tfIn=abi.TF_PQ, inMax=[65535] * 3)
    for gamut in (False, True):
        bound, exact = _bound_and_model(lin, gamut, "srgb")
        with armed(ctx, gamut=gamut):
            got = host.colorConvert(ctx, pq, tfIn=abi.TF_PQ, inMax=[65535] * 3, tfOut=abi.TF_SRGB)
        _close(got, exact, bound, "pq16 gamut %d" % gamut)
    # a grey image comes out as three planes, as with a matrix
    g = data["grey"]
    bound, exact = _bound_and_model([g[0]] * 3, True, "bt709")
    with armed(ctx):
        got = host.colorConvert(ctx, g, tfOut=abi.TF_BT709)
        ten = _tensor(ctx, g, tfOut=abi.TF_BT709)
        png = host.pngSamples(ctx, g, tfOut=abi.TF_BT709)
    assert len(got) == 3 and ten.shape == (3, 67, 83) and png.shape == (67, 83, 3)
    _close(got, exact, bound, "grey")
    assert all(np.array_equal(ten[c].view(np.uint32), got[c].view(np.uint32)) for c in range(3))
    assert len(host.colorConvert(ctx, g, tfOut=abi.TF_BT709)) == 1  # and one plane again once cleared


# ---- the identity setting ----
def test_identity_is_exact(ctx, data):
    """source <= target, unit == target (norm 1) and no gamut step: every exit's bytes are those of the call without tone mapping"""
    v, pq = data[(67, 83)], data["pq16"]
    m = np.array([[0.9, 0.08, 0.02], [0.05, 0.9, 0.05], [0.01, 0.09, 0.9]], F)
    size, box = (9, 7), (3, 2, 60, 50)

    def exits():
        out = {"convert": host.colorConvert(ctx, v, matrix=m, tfOut=abi.TF_SRGB),
               "convert_int": host.colorConvert(ctx, pq, tfIn=abi.TF_PQ, inMax=[65535] * 3, tfOut=abi.TF_LINEAR, maxValue=65535),
               "png8": [host.pngSamples(ctx, v, tfOut=abi.TF_SRGB)], "png16": [host.pngSamples(ctx, v, matrix=m, tfOut=abi.TF_SRGB, bitDepth=16)],
               "f32": [_tensor(ctx, v, tfOut=abi.TF_SRGB)], "u8": [_tensor(ctx, v, dtype="uint8", layout="HWC", tfOut=abi.TF_SRGB)],
               "resized": [_resized(ctx, lambda p: host.tensorResized(ctx, v, None, p, size, box, tfOut=abi.TF_SRGB), size)],
               "batch": [_resized(ctx, lambda p: host.tensorResizedBatch(ctx, [host.tensorBatchItem(size, box, planes=v, tfOut=abi.TF_SRGB),
                                                                             host.tensorBatchItem(size, None, planes=v, tfOut=abi.TF_SRGB)], p), size, n=2)]}
        return out
    plain = exits()
    with armed(ctx, unit=TARGET, source=TARGET, target=TARGET, gamut=False):
        same = exits()
    with armed(ctx, unit=TARGET, source=100.0, target=TARGET, gamut=False):
        below = exits()
    for k in plain:
        for a, b, c in zip(plain[k], same[k], below[k]):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)) and np.array_equal(a.view(np.uint8), c.view(np.uint8)), k
    # and through the image: transform, PNGWriter and toTensor with the identity ToneMap against peak detection off
    ident = ToneMap(TARGET, sourceNits=TARGET, unitNits=TARGET, gamut=False)
    im = JXLImage([a.copy() for a in pq], _info(transfer=TF_PQ, bits=16), _backend(ctx))
    a = im.transform(PRI_SRGB, WP_D65, TF_SRGB, PEAK_DETECT_OFF, device=True)
    b = im.transform(PRI_SRGB, WP_D65, TF_SRGB, device=True, toneMap=ident)
    assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a.buffer, b.buffer))
    for kw in (dict(deviceSamples=True), dict(deviceColor=True)):
        assert np.array_equal(PNGWriter(im, peakDetect=PEAK_DETECT_OFF, **kw).samples, PNGWriter(im, toneMap=ident, **kw).samples)
    for kw in (dict(), dict(size=size, box=box), dict(dtype=torch.uint8, layout="HWC")):
        x, y = im.toTensor(peakDetect=PEAK_DETECT_OFF, **kw), im.toTensor(toneMap=ident, **kw)
        bits = torch.uint8 if x.dtype == torch.uint8 else torch.int32  # (a code value of 0 is NaN behind the reference's PQ curve)
        assert x.shape == y.shape and torch.equal(x.view(bits), y.view(bits)), kw


# ---- one operator everywhere ----
@pytest.mark.parametrize("shape", SHAPES)
def test_integer_exits_quantise_the_devices_own_float_result(ctx, data, shape):
    v = data[shape]
    with armed(ctx):
        f = host.colorConvert(ctx, v, tfOut=abi.TF_SRGB)
        u8 = _tensor(ctx, v, dtype="uint8", layout="HWC", tfOut=abi.TF_SRGB)
        png8 = host.pngSamples(ctx, v, tfOut=abi.TF_SRGB)
        png16 = host.pngSamples(ctx, v, tfOut=abi.TF_SRGB, bitDepth=16, bigEndian=True)
    # the existing quantiser, on a context that is not armed, applied to those float planes
    assert np.array_equal(u8, _tensor(ctx, f, dtype="uint8", layout="HWC"))
    assert np.array_equal(png8, host.pngSamples(ctx, f)) and np.array_equal(u8, png8)
    assert np.array_equal(png16, host.pngSamples(ctx, f, bitDepth=16, bigEndian=True))


def test_resized_and_batched_exits_filter_the_tone_mapped_planes(ctx, data):
    v = data[(67, 83)]
    for size, box, resample, filt in (((9, 7), (3, 2, 60, 50), "triangle", rr.TRIANGLE), ((80, 90), None, "triangle", rr.TRIANGLE), ((5, 4), None, "box", rr.BOX)):
        bx = (0, 0, 83, 67) if box is None else box
        with armed(ctx):
            got = _resized(ctx, lambda p: host.tensorResized(ctx, v, None, p, size, box, resample, tfOut=abi.TF_SRGB), size)[0]
            lin = host.colorConvert(ctx, v)  # the device's own tone-mapped linear planes
        ty, tx = rr.taps(bx[3], size[0], filt), rr.taps(bx[2], size[1], filt)
        with np.errstate(all="ignore"):
            mid = [rr.resample(p, ty, tx, bx) for p in lin]
        exp = host.colorConvert(ctx, mid, tfOut=abi.TF_SRGB)
        for c in range(3):
            ge, ex = got[c], exp[c]
            assert np.array_equal(np.isnan(ge), np.isnan(ex)) and np.array_equal(ge[~np.isnan(ge)].view(np.uint32), ex[~np.isnan(ex)].view(np.uint32)), (size, c)
    # three images from three homes in one batch against three single calls, through the image API
    be = _backend(ctx)
    size = (11, 13)
    a, b, c3 = data[(67, 83)], data[(264, 40)], data[(8, 8)]
    ims = [JXLImage([None] * 3, _info(), be, planeSet=host.DeviceCanvas.fromArrays(ctx, list(a))),
           JXLImage([None] * 3, _info(), be, resident=host.ResidentPlanes.upload(ctx, list(b))),
           JXLImage([x.copy() for x in c3], _info(), be)]
    singles = [im.toTensor(size=size, toneMap=TONE) for im in ims]
    batch = toTensorBatch(ims, size, toneMap=TONE)
    assert not ctx.toneMapArmed() and tuple(batch.shape) == (3, 3) + size
    for i in range(3):
        assert torch.equal(batch[i].view(torch.int32), singles[i].view(torch.int32)), i
    plain = toTensorBatch(ims, size, peakDetect=PEAK_DETECT_OFF)
    assert not torch.equal(batch.view(torch.int32), plain.view(torch.int32))  # (the batch was tone-mapped)
    ims[0].close()


# ---- arming leaves nothing behind ----
def test_arming_leaves_nothing_behind(ctx, data):
    v = data[(67, 83)]
    before = host.colorConvert(ctx, v, tfOut=abi.TF_SRGB)
    peak, pfm = host.determinePeak(ctx, v), host.pfmSamples(ctx, v)
    with armed(ctx):
        assert ctx.toneMapArmed()
        mapped = host.colorConvert(ctx, v, tfOut=abi.TF_SRGB)
        # the peak and the PFM samples do not look at it
        assert host.determinePeak(ctx, v).tobytes() == peak.tobytes() and np.array_equal(host.pfmSamples(ctx, v), pfm)
        # a scale excludes it: refused, nothing written
        p = host.colorParams(list(v), scale=0.5)
        outs = [np.full(v[0].shape, 7.25, F) for _ in range(3)]
        st = ctx.lib.jxl_stage_color_convert(ctx.h, host._pv(list(v)), v[0].size, C.byref(p), host._pv(outs))
        assert st == abi.JXL_ERR_INVALID_ARGUMENT and all(np.all(o == F(7.25)) for o in outs)
        with pytest.raises(_lib.IllegalArgumentException):
            host.pngSamples(ctx, v, scale=0.5)
        with pytest.raises(_lib.IllegalArgumentException):
            _tensor(ctx, v, scale=0.5)
        # integer output through a linear curve is fine while armed
        assert host.colorConvert(ctx, v, maxValue=255)[0].dtype == np.int32
    assert not ctx.toneMapArmed()
    after = host.colorConvert(ctx, v, tfOut=abi.TF_SRGB)
    assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(before, after))
    assert not all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(before, mapped))
    # a bad block is refused and changes nothing; the scale works again
    for bad in (dict(unit=0.0), dict(source=20000.0), dict(target=float("nan")), dict(lum=[0.0, 0.0, 0.0]), dict(lum=[1.0, 1.0, 0.5])):
        with pytest.raises(_lib.IllegalArgumentException):
            with armed(ctx, **bad):
                pass
        assert not ctx.toneMapArmed()
    t = host.toneMapParams(LUM, UNIT, SOURCE, TARGET)
    t.gamut = 2
    with pytest.raises(_lib.IllegalArgumentException):
        host.setToneMap(ctx, t)
    assert host.colorConvert(ctx, v, scale=0.5)[0].dtype == np.float32
    # an exception between arming and clearing: the image API clears all the same
    be = _backend(ctx)

    def broken(*a, **kw):
        assert ctx.toneMapArmed()
        raise RuntimeError("the call in between failed")
    be.tensor_samples = broken
    im = JXLImage([x.copy() for x in v], _info(), be)
    with pytest.raises(RuntimeError):
        im.toTensor(toneMap=TONE)
    assert not ctx.toneMapArmed()
    again = host.colorConvert(ctx, v, tfOut=abi.TF_SRGB)
    assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(before, again))
