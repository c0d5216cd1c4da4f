"""No GPU: the decisions PNGWriter(deviceSamples=True) shares with JXLImage._transform_device come out of one function
(JXLImage._color_plan) and are the ones _transform_device took before it was factored out -- checked against a restatement of
that earlier code on the image cases of tests/test_color_gpu.py, with a backend that records its calls; and the CLI knows
--device-png."""
import types

import numpy as np
import pytest

from jxlatte_amd import __main__ as cli
from jxlatte_amd import decoder
from jxlatte_amd.decoder import (CE_GRAY, CE_RGB, PEAK_DETECT_AUTO, PEAK_DETECT_OFF, PEAK_DETECT_ON, PRI_BT2100, PRI_P3, PRI_SRGB, TF_BT709,
                                 TF_LINEAR, TF_PQ, TF_SRGB, WP_D65, JXLImage, PNGWriter, get_conversion_matrix)

F = np.float32


def _info(gray=False, bits=8, transfer=TF_SRGB, prim=PRI_SRGB, use_icc=False):
    return types.SimpleNamespace(colour_space=CE_GRAY if gray else CE_RGB, num_extra=0, ec_type=[], ec_alpha_associated=[], ec_bits=[],
                                 prim_xy=list(prim), white_xy=list(WP_D65), transfer=transfer, xyb_encoded=False,
                                 bits_per_sample=bits, use_icc=use_icc)


def _image_cases():
    """the images of test_color_gpu._image_cases (that module is GPU-only), smaller"""
    rng = np.random.default_rng(42)
    shape = (6, 10)
    pq = [rng.uniform(0.2, 0.6, shape).astype(F) for _ in range(3)]
    return {
        "p3-int8": ([rng.integers(0, 256, shape).astype(np.int32) for _ in range(3)], _info(prim=PRI_P3)),
        "bt709-float": ([rng.uniform(0, 1, shape).astype(F) for _ in range(3)], _info(transfer=TF_BT709, bits=16)),
        "pq-bt2100": (pq, _info(transfer=TF_PQ, prim=PRI_BT2100, bits=16)),
        "grey-gamma-int16": ([rng.integers(0, 65536, shape).astype(np.int32)], _info(gray=True, bits=16, transfer=4545455, prim=PRI_P3)),
        "grey-gamma-int16-same-primaries": ([rng.integers(0, 65536, shape).astype(np.int32)], _info(gray=True, bits=16, transfer=4545455)),
        "grey-pq-float": ([rng.uniform(0.2, 0.6, shape).astype(F)], _info(gray=True, bits=16, transfer=TF_PQ, prim=PRI_BT2100)),
        "srgb-int8": ([rng.integers(0, 256, shape).astype(np.int32) for _ in range(3)], _info()),
        "linear-int16": ([rng.integers(0, 65536, shape).astype(np.int32) for _ in range(3)], _info(bits=16, transfer=TF_LINEAR)),
        "mixed": ([rng.integers(0, 256, shape).astype(np.int32), rng.uniform(0, 1, shape).astype(F), rng.integers(0, 256, shape).astype(np.int32)],
                  _info(transfer=TF_LINEAR)),
    }


class Recorder:
    """a backend that records what it is asked and answers with planes of the right count"""

    def __init__(self, peak):
        self.calls, self.peak = [], F(peak)

    @staticmethod
    def _norm(planes, params):
        kw = {k: (None if v is None else np.asarray(v).tolist()) for k, v in sorted(params.items())}
        return [(p.dtype.str, p.tobytes()) for p in planes], kw

    def color_peak(self, planes, **params):
        self.calls.append(("peak",) + tuple(self._norm(planes, params)))
        return self.peak

    def color_convert(self, planes, **params):
        self.calls.append(("convert",) + tuple(self._norm(planes, params)))
        n = 3 if (len(planes) == 3 or params.get("matrix") is not None) else 1
        return [np.zeros(planes[0].shape, F) for _ in range(n)]

    def pack(self, planes, bit_depth, alpha, premultiplied, tagged, big_endian):
        self.calls.append(("pack", len(planes), alpha is not None))
        return np.zeros(planes[0].shape + (len(planes) + (alpha is not None),), np.uint8 if bit_depth == 8 else np.uint16)

    def png_samples(self, planes, alpha, **params):
        self.calls.append(("png", alpha is not None) + tuple(self._norm(planes, params)))
        n = (3 if (len(planes) == 3 or params.get("matrix") is not None) else 1) + (alpha is not None)
        return np.zeros(planes[0].shape + (n,), np.uint8 if params["bitDepth"] == 8 else np.uint16)


def _before(im, primaries, whitePoint, transfer, peakDetect):
    """JXLImage._transform_device's calls as that function made them before the decisions moved to _color_plan (restated from it)"""
    be = im.backend
    tone_map = not (decoder._prim_matches(primaries, im.primariesXY) and decoder._xy_matches(whitePoint, im.whiteXY))
    if not tone_map and transfer == im.transfer_:
        return
    tf_in, gamma_in = decoder._tf_selector(im.transfer_)
    tf_out, gamma_out = decoder._tf_selector(transfer)
    colors = im.getColorChannelCount()
    depth_max = [(1 << im.bitDepths[c]) - 1 for c in range(colors)]
    planes = [im.buffer[c] for c in range(colors)]
    if len({p.dtype for p in planes}) != 1:
        cast_max = depth_max if (im.transfer_ != TF_LINEAR or tone_map) else None
        planes = [im._as_float(c) if cast_max else im._as_float(c, with_depth=False) for c in range(colors)]
    front = dict(tfIn=tf_in, gammaIn=gamma_in)
    if tone_map:
        front["matrix"] = get_conversion_matrix(primaries, whitePoint, im.primariesXY, im.whiteXY)
    if tone_map and transfer == TF_LINEAR:
        be.color_convert(planes, inMax=depth_max, **front)
        return
    scale = None
    if im.taggedTransfer == TF_PQ and peakDetect in (PEAK_DETECT_AUTO, PEAK_DETECT_ON):
        to_pq = transfer in (TF_PQ, TF_LINEAR)
        from_pq = tone_map or im.transfer_ in (TF_PQ, TF_LINEAR)
        if from_pq and not to_pq:
            s = F(F(1) / be.color_peak(planes, inMax=depth_max, **front))
            if s > 1.0 or peakDetect == PEAK_DETECT_ON:
                scale = s
    first_max = depth_max if (im.transfer_ != TF_LINEAR or tone_map or scale is not None) else [im.bitDepths[c] for c in range(colors)]
    be.color_convert(planes, inMax=first_max, scale=scale, tfOut=tf_out, gammaOut=gamma_out, **front)


TARGETS = [(PRI_SRGB, TF_SRGB), (PRI_BT2100, TF_PQ), (PRI_SRGB, TF_LINEAR), (PRI_P3, TF_LINEAR), (PRI_P3, TF_BT709)]


@pytest.mark.parametrize("name", sorted(_image_cases()))
def test_the_shared_plan_takes_the_decisions_transform_device_took(name):
    buf, info = _image_cases()[name]
    n = 0
    for (prim, tf), detect, peak in [(t, d, p) for t in TARGETS for d in (PEAK_DETECT_AUTO, PEAK_DETECT_ON, PEAK_DETECT_OFF) for p in (0.5, 2.0)]:
        old, new = Recorder(peak), Recorder(peak)
        _before(JXLImage([b.copy() for b in buf], info, old), prim, WP_D65, tf, detect)
        out = JXLImage([b.copy() for b in buf], info, new).transform(prim, WP_D65, tf, detect, device=True)
        assert new.calls == old.calls, (name, tf, detect, peak)
        assert (out.transfer_ == tf) and len([c for c in new.calls if c[0] == "convert"]) <= 1
        n += 1
    assert n == 30


@pytest.mark.parametrize("name", sorted(_image_cases()))
@pytest.mark.parametrize("hdr", [False, True])
def test_device_samples_asks_for_the_same_stages_in_one_call(name, hdr):
    """PNGWriter(deviceSamples=True): at most one peak call, then ONE png_samples call whose colour keywords are those of the
    color_convert call PNGWriter(deviceColor=True) makes (every stage off where that path leaves the image as it is); a grey
    image that is tone-mapped keeps the passes one by one"""
    buf, info = _image_cases()[name]
    a, b = Recorder(0.5), Recorder(0.5)
    im = JXLImage([x.copy() for x in buf], info, a)
    im.transform(PRI_BT2100 if hdr else PRI_SRGB, WP_D65, TF_PQ if hdr else TF_SRGB, PEAK_DETECT_AUTO, device=True)
    w = PNGWriter(JXLImage([x.copy() for x in buf], info, b), hdr=hdr, deviceSamples=True)
    png = [c for c in b.calls if c[0] == "png"]
    conv = [c for c in a.calls if c[0] == "convert"]
    grey_tone_map = info.colour_space == CE_GRAY and conv and conv[0][2].get("matrix") is not None
    if grey_tone_map:
        assert not png and w.bus_bytes is None and [c[0] for c in b.calls] == [c[0] for c in a.calls] + ["pack"]
        assert len([c for c in b.calls if c[0] == "peak"]) <= 1
        return
    assert len(png) == 1 and len([c for c in b.calls if c[0] == "peak"]) == len([c for c in a.calls if c[0] == "peak"]) <= 1
    assert not [c for c in b.calls if c[0] == "convert"]
    kw = dict(png[0][3])
    extra = {k: kw.pop(k) for k in ("premultiplied", "bitDepth", "bigEndian", "alphaDepth", "colorDepth")}
    assert extra["bitDepth"] == w.bitDepth and extra["bigEndian"] is True and extra["premultiplied"] is False
    if conv:
        assert png[0][2] == conv[0][1] and kw == conv[0][2], name
    else:  # the image as it is
        colors = len(buf)
        assert kw == dict(inMax=[(1 << info.bits_per_sample) - 1] * colors), name
    # bytes up: the planes of the one call, and before it those the peak reads (all three under a matrix, else determinePeak's one)
    up = sum(x.nbytes for x in png_planes(png[0]))
    for c in b.calls:
        if c[0] == "peak":
            pl = [np.frombuffer(raw, np.dtype(dt)) for dt, raw in c[1]]
            up += sum(x.nbytes for x in pl) if c[2].get("matrix") is not None else pl[min(1, len(pl) - 1)].nbytes
    assert w.samples.shape == buf[0].shape + (len(buf),) and w.bus_bytes == (up, w.samples.nbytes)


def png_planes(call):
    return [np.frombuffer(raw, np.dtype(dt)) for dt, raw in call[2]]


def test_an_icc_image_goes_through_with_every_colour_stage_off():
    buf, _ = _image_cases()["p3-int8"]
    be = Recorder(0.5)
    w = PNGWriter(JXLImage([x.copy() for x in buf], _info(prim=PRI_P3, use_icc=True), be), deviceSamples=True)
    assert [c[0] for c in be.calls] == ["png"] and be.calls[0][3] == dict(
        alphaDepth=None, bigEndian=True, bitDepth=8, colorDepth=8, inMax=[255, 255, 255], premultiplied=False)
    assert w.has_icc and w.colorMode == 2


def test_a_backend_without_png_samples_is_an_error():
    buf, info = _image_cases()["srgb-int8"]
    be = types.SimpleNamespace()
    with pytest.raises(TypeError):
        PNGWriter(JXLImage(buf, info, be), deviceSamples=True)


def test_cli_parses_device_png():
    a = cli.parser().parse_args(["in.jxl", "out.png", "--device-png"])
    assert a.device_png and not a.device_color and a.input == "in.jxl" and a.output == "out.png"
    assert not cli.parser().parse_args(["in.jxl"]).device_png
