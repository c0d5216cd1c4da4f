"""GPU: JXLDecoder(device_canvas=True, device_frames=True) -- Modular frames reach the resident canvas as plane sets made from the
Modular context -- against the default decoder on every committed bitstream: planes (dtype, shape, bits) and the PNG's samples,
equality everywhere (NaNs compared as one value, as tests/test_canvas_gpu.py does); which route each frame takes; what crosses the
bus; which backend hooks run. The default decode of a sample is made once per (sample, orientation, device_splines) and shared:
device_splines is part of the reference because the device's spline samples are its own (include/jxlatte_amd.h)."""
import collections
import glob
import os
import zlib

import numpy as np
import pytest

from conftest import assert_bits_equal
from jxlatte_amd import decoder as D
from jxlatte_amd import host
from jxlatte_amd.decoder import DeviceBackend, JXLDecoder, PNGWriter

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAMPLES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "samples", "*.jxl")))
NAMES = [os.path.splitext(os.path.basename(p))[0] for p in SAMPLES]
SET = "device set (modular)"
HOOKS = ("rct", "squeeze", "upsample", "modular_to_float", "keep_planes")
PIXELS = {"blendmodes_5": 1024 * 1024, "wb-rainbow": 1024 * 576}  # of one frame, before upsampling


class CountingBackend(DeviceBackend):
    """the device backend on the session's context, with counters around the hooks a qualifying frame must not reach"""

    def __init__(self, ctx):
        self.host, self.ctx = host, ctx
        self.palette_log = []
        self.calls = collections.Counter()


for _name in HOOKS:
    def _counted(self, *a, _name=_name, **kw):
        self.calls[_name] += 1
        return getattr(DeviceBackend, _name)(self, *a, **kw)
    setattr(CountingBackend, _name, _counted)


@pytest.fixture(scope="module")
def backend(ctx):
    return CountingBackend(ctx)


def _path(name):
    return SAMPLES[NAMES.index(name)]


def _decode(path, backend, orientation=None, trace=None, **kw):
    dec = JXLDecoder(path, backend=backend, **kw)
    if orientation is not None:
        dec.info.orientation = orientation
    if trace is not None:
        dec.trace = trace
    backend.calls.clear()
    return dec, dec.decode()


def _reference(backend, name, orientation=None, device_splines=False):
    """the default decoder's image as (planes, PNGWriter(deviceColor=True), stats)"""
    key = (name, orientation, device_splines)
    if key not in _reference.cache:
        dec, im = _decode(_path(name), backend, orientation, device_splines=device_splines)
        assert [s["frame"] for s in dec.stats] == ["host: device_frames is off"] * len(dec.stats)
        planes = im.getBuffer()
        for a in planes:
            a.setflags(write=False)
        _reference.cache[key] = (planes, PNGWriter(im, deviceColor=True), dec.stats)
        dec.close()
    return _reference.cache[key]


_reference.cache = {}


def _check_image(backend, name, im, orientation=None, device_splines=False):
    """the writer first (while the planes are the image's), then the planes"""
    exp_planes, r, _ = _reference(backend, name, orientation, device_splines)
    w = PNGWriter(im, deviceSamples=True)
    assert (w.bitDepth, w.colorMode, w.width, w.height) == (r.bitDepth, r.colorMode, r.width, r.height), name
    assert w.samples.dtype == r.samples.dtype and w.samples.shape == r.samples.shape, name
    assert np.array_equal(w.samples, r.samples), "%s: %d PNG samples differ" % (name, int((w.samples != r.samples).sum()))
    buf = im.getBuffer()
    assert len(buf) == len(exp_planes)
    for c in range(len(buf)):
        assert buf[c].dtype == exp_planes[c].dtype and buf[c].shape == exp_planes[c].shape, (name, c, buf[c].dtype, exp_planes[c].dtype)
        assert_bits_equal(buf[c], exp_planes[c], "%s plane %d" % (name, c), any_nan=True)


@pytest.mark.parametrize("device_image", [False, True], ids=["", "image"])
@pytest.mark.parametrize("device_splines", [False, True], ids=["host-splines", "device-splines"])
@pytest.mark.parametrize("name", ["blendmodes_5", "wb-rainbow"])
def test_the_multi_frame_samples_equal_the_default_decoder(backend, name, device_splines, device_image):
    _reference(backend, name, None, device_splines)  # (first: a default decode takes the context's resident planes)
    dec, im = _decode(_path(name), backend, device_canvas=True, device_frames=True, device_splines=device_splines, device_image=device_image)
    try:
        print(name, [s["frame"] for s in dec.stats], [s.get("plane_moves") for s in dec.stats], [s["blend_bus"] for s in dec.stats])
        assert [s["frame"] for s in dec.stats] == [SET] * 5  # a frame that falls to the host fails the test
        assert [s["canvas"] for s in dec.stats] == ["device"] * 5
        assert (im.planeSet is not None) == device_image
        _check_image(backend, name, im, None, device_splines)
    finally:
        dec.close()


@pytest.mark.parametrize("name", ["blendmodes_5", "wb-rainbow"])
def test_bus_traffic_and_hooks(backend, name):
    """with device_splines every stage of every frame is a device stage: the encoded channels (RGB + alpha, int32) go up once per
    frame, nothing comes down, no plane moves, and the hooks of the host route are never called"""
    dec, im = _decode(_path(name), backend, device_canvas=True, device_frames=True, device_splines=True)
    try:
        assert [s["frame"] for s in dec.stats] == [SET] * 5
        assert [s["blend_bus"] for s in dec.stats] == [(4 * 4 * PIXELS[name], 0)] * 5
        for s in dec.stats:
            assert "h2d" not in s["plane_moves"] and "d2h" not in s["plane_moves"], s["plane_moves"]
        assert {h: backend.calls[h] for h in HOOKS} == {h: 0 for h in HOOKS}
    finally:
        dec.close()
    if name == "wb-rainbow":  # splines on the host: frames 1 and 4 bring their colour planes down and up, and say so; the alpha never moves
        dec, im = _decode(_path(name), backend, device_canvas=True, device_frames=True)
        try:
            assert [s["frame"] for s in dec.stats] == [SET] * 5
            assert [s["plane_moves"] for s in dec.stats] == [[], ["d2h", "h2d"], [], [], ["d2h", "h2d"]]
            plane = 4 * PIXELS[name]
            assert [s["blend_bus"] for s in dec.stats] == [(4 * plane + (3 * plane if k in (1, 4) else 0), 0) for k in range(5)]
            assert backend.calls["rct"] == backend.calls["squeeze"] == backend.calls["upsample"] == backend.calls["modular_to_float"] == 0
        finally:
            dec.close()


@pytest.mark.parametrize("name", ["blendmodes_5", "wb-rainbow"])
def test_switch_off(backend, name, monkeypatch):
    """device_canvas alone: the front-end is never told to defer, the host route's hooks run, every frame's planes go up for the blend"""
    defers = []
    real = D.frontend.Frontend.set_defer_transforms
    monkeypatch.setattr(D.frontend.Frontend, "set_defer_transforms", lambda self, on: (defers.append(on), real(self, on))[1])
    dec, im = _decode(_path(name), backend, device_canvas=True, device_splines=True)
    try:
        assert defers == []
        assert [s["frame"] for s in dec.stats] == ["host: device_frames is off"] * 5
        assert [s["canvas"] for s in dec.stats] == ["device"] * 5
        if name == "blendmodes_5":  # per frame: one RCT through the hook, four int32 planes up for the blend
            assert backend.calls["rct"] == 5 and backend.calls["keep_planes"] == 0
            assert [s["blend_bus"] for s in dec.stats] == [(4 * 4 * PIXELS[name], 0)] * 5
        else:  # frames 0 and 3 have an RCT; frame 0's alpha is upsampled on its own; frames 0, 1 and 4 are cast and uploaded
            assert backend.calls["rct"] == 2 and backend.calls["upsample"] == 1 and backend.calls["keep_planes"] == 3
        _check_image(backend, name, im, None, True)
    finally:
        dec.close()
    dec, im = _decode(_path(name), backend, device_frames=True)  # the switch without a device canvas does nothing but say so
    try:
        assert [s["frame"] for s in dec.stats] == ["host: device_canvas is off"] * 5
        assert [s["canvas"] for s in dec.stats] == ["host"] * 5
        _check_image(backend, name, im)
    finally:
        dec.close()


def test_landing_on_frame_2(backend, monkeypatch):
    """the type plan lands on frame 2: that frame's planes come down from its set, the host blends, and the image is the default's"""
    real, calls = D.blend_type_plan, []

    def plan(*a, **kw):
        p = real(*a, **kw)
        calls.append(p.verdict)
        if len(calls) == 3:
            p.verdict = "land: the test says so"
        return p
    monkeypatch.setattr(D, "blend_type_plan", plan)
    name = "wb-rainbow"
    _reference(backend, name, None, True)
    calls.clear()
    dec, im = _decode(_path(name), backend, device_canvas=True, device_frames=True, device_splines=True)
    try:
        assert calls[:3] == ["device"] * 3 and len(calls) == 3
        assert [s["frame"] for s in dec.stats] == [SET, SET, SET] + ["host: the canvas has landed (the test says so)"] * 2
        assert [s["canvas"] for s in dec.stats] == ["device", "device"] + ["landed: the test says so"] * 3
        _check_image(backend, name, im, None, True)
    finally:
        dec.close()


@pytest.mark.parametrize("orientation", [3, 6])
def test_orientation_forced_on_wb_rainbow(backend, orientation):
    name = "wb-rainbow"
    _reference(backend, name, orientation, True)
    dec, im = _decode(_path(name), backend, orientation, device_canvas=True, device_frames=True, device_splines=True)
    try:
        assert [s["frame"] for s in dec.stats] == [SET] * 5
        assert (im.getHeight(), im.getWidth()) == ((1152, 2048) if orientation == 3 else (2048, 1152))
        _check_image(backend, name, im, orientation, True)
    finally:
        dec.close()


@pytest.mark.parametrize("name", ["blendmodes_5", "wb-rainbow"])
def test_a_trace_listener_takes_the_host_route(backend, name):
    def listener(log):
        return lambda k, stage, planes, fused: log.append((k, stage, fused, [(p.dtype.str, p.shape, zlib.crc32(np.ascontiguousarray(p).tobytes()))
                                                                              for p in planes]))
    want, got = [], []
    ref, _ = _decode(_path(name), backend, trace=listener(want))
    ref.close()
    dec, im = _decode(_path(name), backend, trace=listener(got), device_canvas=True, device_frames=True)
    try:
        assert [s["frame"] for s in dec.stats] == ["host: a trace listener is set"] * 5
        assert len(want) > 5 and got == want
        _check_image(backend, name, im)
    finally:
        dec.close()


@pytest.mark.parametrize("name", [n for n in NAMES if n not in ("blendmodes_5", "wb-rainbow")])
def test_every_other_sample(backend, name):
    _reference(backend, name)
    dec, im = _decode(_path(name), backend, device_canvas=True, device_frames=True)
    try:
        routes = [s["frame"] for s in dec.stats]
        print(name, routes, [s["canvas"] for s in dec.stats])
        if name in ("art", "quilt"):
            assert routes == [SET] and dec.stats[0]["canvas"] == "device"
            assert {h: backend.calls[h] for h in HOOKS} == {h: 0 for h in HOOKS}
        elif name == "patches-lossless":
            assert routes == ["host: a Palette in the frame-level chain"] * 2
        else:
            assert routes == ["host: not a Modular frame"] * len(routes)
        _check_image(backend, name, im)
    finally:
        dec.close()
