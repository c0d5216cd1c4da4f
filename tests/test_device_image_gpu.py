"""GPU: JXLDecoder(device_image=True) on every committed bitstream against the default decoder -- planes (dtype, shape, bits), the
PNG's samples and metadata for both `hdr` values against PNGWriter(deviceColor=True), the PFM's bytes against the host PFMWriter --
alone, with device_canvas and with device_output; which route each image takes; and what crosses the bus. Equality everywhere
(NaNs compared as one value, as tests/test_canvas_gpu.py does). The default decode of a sample is made once and shared."""
import glob
import os

import numpy as np
import pytest

from conftest import assert_bits_equal
from jxlatte_amd import frontend, host
from jxlatte_amd.decoder import DeviceBackend, JXLDecoder, PFMWriter, PNGWriter

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAMPLES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "samples", "*.jxl")))
NAMES = [os.path.splitext(os.path.basename(p))[0] for p in SAMPLES]
CONFIGS = {"image": dict(device_image=True), "image+canvas": dict(device_image=True, device_canvas=True),
           "image+output": dict(device_image=True, device_output=True)}
MODULAR_FRAME, CANVAS = "device set (modular frame)", "device set (canvas)"


@pytest.fixture(scope="module")
def backend(ctx):
    be = DeviceBackend.__new__(DeviceBackend)
    be.host, be.ctx = host, ctx
    be.palette_log = []
    return be


def _path(name):
    return SAMPLES[NAMES.index(name)]


def _decode(path, backend, orientation=None, **kw):
    dec = JXLDecoder(path, backend=backend, **kw)
    if orientation is not None:
        dec.info.orientation = orientation
    return dec, dec.decode()


def _reference(backend, name, orientation=None):
    """the default decoder's image as (planes, {hdr: PNGWriter(deviceColor=True)}, PFM samples); made once per (sample, orientation)"""
    key = (name, orientation)
    if key not in _reference.cache:
        dec, im = _decode(_path(name), backend, orientation)
        assert [s["image"] for s in dec.stats] == ["host: device_image is off"] * len(dec.stats)
        assert not im.onDevice() and im.planeSet is None
        planes = im.getBuffer()
        for a in planes:
            a.setflags(write=False)
        _reference.cache[key] = (planes, {hdr: PNGWriter(im, hdr=hdr, deviceColor=True) for hdr in (False, True)}, PFMWriter(im).samples)
        dec.close()
    return _reference.cache[key]


_reference.cache = {}


def _check_image(backend, name, dec, im, orientation=None, expect_bus=None):
    """writers first (while the planes are the image's), then the planes"""
    exp_planes, exp_png, exp_pfm = _reference(backend, name, orientation)
    writers = {hdr: PNGWriter(im, hdr=hdr, deviceSamples=True) for hdr in (False, True)}
    pfm = PFMWriter(im, deviceSamples=True)
    for hdr, w in writers.items():
        r = exp_png[hdr]
        assert (w.bitDepth, w.colorMode, w.width, w.height, w.has_icc, w.hdr) == (r.bitDepth, r.colorMode, r.width, r.height, r.has_icc, r.hdr), (name, hdr)
        assert w.samples.dtype == r.samples.dtype and w.samples.shape == r.samples.shape, (name, hdr)
        assert np.array_equal(w.samples, r.samples), "%s hdr %d: %d samples differ" % (name, hdr, int((w.samples != r.samples).sum()))
        if expect_bus:
            assert w.bus_bytes == (0, w.samples.nbytes), (name, hdr, w.bus_bytes)
    assert (pfm.width, pfm.height, pfm.gray) == (im.getWidth(), im.getHeight(), False)
    assert pfm.samples.shape == exp_pfm.shape and np.array_equal(pfm.samples, exp_pfm), "%s: PFM bytes differ" % name
    if expect_bus:
        assert pfm.bus_bytes == (0, pfm.samples.nbytes), (name, pfm.bus_bytes)
    buf = im.getBuffer()
    assert len(buf) == len(exp_planes)
    for c in range(len(buf)):
        assert buf[c].dtype == exp_planes[c].dtype and buf[c].shape == exp_planes[c].shape, (name, c, buf[c].dtype, exp_planes[c].dtype)
        assert_bits_equal(buf[c], exp_planes[c], "%s plane %d" % (name, c), any_nan=True)
    assert im.getBuffer(False) is im.getBuffer(False)  # downloaded once, cached


@pytest.mark.parametrize("config", sorted(CONFIGS))
@pytest.mark.parametrize("name", NAMES)
def test_every_sample_equals_the_default_decoder(backend, name, config):
    _reference(backend, name)  # (first: a default decode may take the context's resident planes from an image made before it)
    dec, im = _decode(_path(name), backend, **CONFIGS[config])
    try:
        route = dec.stats[-1]["image"]
        print(name, config, [s["image"] for s in dec.stats])
        on_set = route in (MODULAR_FRAME, CANVAS)
        assert on_set == (im.planeSet is not None) and (on_set or route.startswith("host: ")), route
        if name in ("art", "quilt"):
            assert route == MODULAR_FRAME and len(dec.stats) == 1
        elif name in ("blendmodes_5", "wb-rainbow"):
            if config == "image+canvas":
                assert route == CANVAS and [s["canvas"] for s in dec.stats] == ["device"] * 5
            else:
                assert route.startswith("host: "), route
        elif name == "patches-lossless":
            assert route.startswith("host: ") and "Palette" in route, route
        else:  # the VarDCT images
            assert route == "host: not a Modular frame" or (config == "image+canvas" and route == CANVAS), route
            if config == "image+output":  # device_output's direct path is unchanged and comes first
                assert im.planeSet is None and (dec.stats[-1]["output"] == "device") == (im.resident is not None)
                if name in ("lenna", "bbb"):
                    assert im.resident is not None
        if on_set:
            assert im.onDevice() and im.setLive() and im.planeSet.shape == (im.getHeight(), im.getWidth())
            assert len(im.planeSet) == 3 + dec.info.num_extra
        _check_image(backend, name, dec, im, expect_bus=on_set)
        if on_set:
            ps = im.planeSet
            clone = im._clone()
            assert clone.planeSet is None and not clone.onDevice()  # a clone lands on the host
            im.close()
            assert ps.id is None and not im.setLive() and len(im.getBuffer()) == len(ps)  # the host arrays stay
    finally:
        dec.close()


def _encoded_bytes(name):
    fe = frontend.Frontend(open(_path(name), "rb").read())
    try:
        fe.set_defer_transforms(True)
        fe.next_frame(None, None, None)
        return sum(4 * fe.modular_channel(i)[0].size for i in range(fe.modular_channel_count()))
    finally:
        fe.close()


@pytest.mark.parametrize("name", ["art", "quilt"])
def test_modular_frame_route_moves_the_encoded_channels_up_and_only_samples_down(backend, name):
    enc = _encoded_bytes(name)
    if name == "art":
        assert enc == 3 * 128 * 128 * 4
    ctx = backend.ctx
    ctx.blend_bus = [0, 0]
    dec, im = _decode(_path(name), backend, device_image=True)
    try:
        assert dec.stats[-1]["image"] == MODULAR_FRAME
        assert dec.stats[-1]["blend_bus"] == (enc, 0) and ctx.blend_bus == [enc, 0]  # one upload, no plane download
        w = PNGWriter(im, deviceSamples=True)
        assert w.bus_bytes == (0, w.samples.nbytes) and ctx.blend_bus == [enc, w.samples.nbytes]
        p = PFMWriter(im, deviceSamples=True)
        assert p.bus_bytes == (0, p.samples.nbytes) and ctx.blend_bus == [enc, w.samples.nbytes + p.samples.nbytes]
        assert [a is None for a in im._buffer] == [True] * len(im._buffer)  # nothing has been downloaded
    finally:
        im.close()
        dec.close()


@pytest.mark.parametrize("orientation", [3, 6])
def test_forced_orientation_on_art(backend, orientation):
    _reference(backend, "art", orientation)
    dec, im = _decode(_path("art"), backend, orientation, device_image=True)
    try:
        assert dec.stats[-1]["image"] == MODULAR_FRAME and (im.getHeight(), im.getWidth()) == (128, 128)
        _check_image(backend, "art", dec, im, orientation, expect_bus=True)
    finally:
        im.close()
        dec.close()


def test_a_second_decode_leaves_the_first_images_set_intact(backend):
    """sets do not share the resident planes' single-owner rule"""
    _reference(backend, "art"), _reference(backend, "quilt")
    d1, im1 = _decode(_path("art"), backend, device_image=True)
    d2, im2 = _decode(_path("quilt"), backend, device_image=True)
    d3, im3 = _decode(_path("lenna"), backend, device_image=True, device_output=True)  # (takes the context's resident planes)
    try:
        assert im1.setLive() and im2.setLive() and im1.planeSet.id != im2.planeSet.id
        _check_image(backend, "quilt", d2, im2, expect_bus=True)
        _check_image(backend, "art", d1, im1, expect_bus=True)
    finally:
        for im in (im1, im2, im3):
            im.close()
        for d in (d1, d2, d3):
            d.close()


def test_a_trace_listener_gets_copies_and_the_set_stays(backend):
    dec = JXLDecoder(_path("art"), backend=backend, device_image=True)
    seen = {}
    dec.trace = lambda k, stage, planes, fused: seen.setdefault(stage, [np.array(p, copy=True) for p in planes])
    im = dec.decode()
    try:
        assert dec.stats[-1]["image"] == MODULAR_FRAME and im.setLive() and set(seen) == {"mod", "xyb"}
        exp = _reference(backend, "art")[0]
        for c in range(3):
            assert_bits_equal(seen["xyb"][c], exp[c], "xyb cut, plane %d" % c)
            assert_bits_equal(seen["mod"][c][:128, :128], exp[c], "mod cut, channel %d" % c)
    finally:
        im.close()
        dec.close()
