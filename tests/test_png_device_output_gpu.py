"""JXLDecoder(device_output=True) + PNGWriter(deviceSamples=True) on the committed bitstreams: the same PNG samples, metadata and
host buffers as the default decoder with PNGWriter(deviceColor=True); the frames that are the whole image really stay on the
device (no download of the planes, only the samples cross the bus); the others take the host arrays through
jxl_stage_png_samples."""
import glob
import io
import os

import numpy as np
import pytest

from conftest import assert_bits_equal
from jxlatte_amd.decoder import DeviceBackend, JXLDecoder, PNGWriter

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAMPLES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "samples", "*.jxl")))
NAMES = [os.path.splitext(os.path.basename(p))[0] for p in SAMPLES]
# the single-frame VarDCT images whose one frame is the image: they must take the direct path
DIRECT = {"lenna", "bbb"}
results = {}


@pytest.fixture(scope="module")
def backend(ctx):
    from jxlatte_amd import host
    be = DeviceBackend.__new__(DeviceBackend)
    be.host, be.ctx = host, ctx
    return be


def _decode(path, backend, orientation=None, **kw):
    dec = JXLDecoder(path, backend=backend, **kw)
    if orientation is not None:
        dec.info.orientation = orientation
    return dec, dec.decode()


def _compare(path, backend, orientation=None):
    name = os.path.basename(path)
    # the device image first: its planes are the backend's resident planes until the next decode
    dec, im = _decode(path, backend, orientation, device_output=True)
    out = dec.stats[-1]["output"]
    writers = {}
    for hdr in (False, True):
        writers[hdr] = PNGWriter(im, hdr=hdr, deviceSamples=True)
    if out == "device":
        assert im.onDevice() and "d2h" not in dec.stats[-1]["plane_moves"], name
        for hdr, w in writers.items():
            a = im.getAlphaIndex()
            up = im.extraChannel(a).nbytes if a >= 0 else 0
            assert w.bus_bytes == (up, w.height * w.width * w.samples.shape[2] * w.bitDepth // 8), (name, hdr, w.bus_bytes)
    else:
        assert out == "host" and not im.onDevice(), name
    buf = im.getBuffer()
    ref_dec, ref_im = _decode(path, backend, orientation)
    assert ref_dec.stats[-1]["output"] == "host"
    exp = ref_im.getBuffer()
    assert len(buf) == len(exp)
    for c in range(len(buf)):
        assert buf[c].dtype == exp[c].dtype and buf[c].shape == exp[c].shape, (name, c)
        assert_bits_equal(buf[c], exp[c], "%s plane %d" % (name, c), any_nan=True)
    for hdr, w in writers.items():
        r = PNGWriter(ref_im, hdr=hdr, deviceColor=True)
        assert (w.bitDepth, w.colorMode, w.width, w.height) == (r.bitDepth, r.colorMode, r.width, r.height), (name, hdr)
        assert w.samples.dtype == r.samples.dtype and w.samples.shape == r.samples.shape, (name, hdr)
        assert np.array_equal(w.samples, r.samples), "%s hdr %d: %d samples differ" % (name, hdr, int((w.samples != r.samples).sum()))
    return out


@pytest.mark.parametrize("path", SAMPLES, ids=NAMES)
def test_every_sample_same_bytes_metadata_and_buffers(backend, path):
    name = os.path.splitext(os.path.basename(path))[0]
    results[name] = _compare(path, backend)
    if name in DIRECT:
        assert results[name] == "device", "%s did not take the direct path" % name


def test_the_direct_path_is_taken_and_the_others_report_host(backend):
    """(runs after the sweep above, in file order; decodes what it needs itself when run alone)"""
    for name in sorted(DIRECT | {"blendmodes_5"}):
        if name not in results:
            results[name] = _compare(os.path.join(ROOT, "tests", "golden", "samples", name + ".jxl"), backend)
    direct = sorted(n for n, o in results.items() if o == "device")
    print("direct path: %s; host path: %s" % (direct, sorted(n for n, o in results.items() if o == "host")))
    assert len(direct) >= 2 and DIRECT <= set(direct)
    assert results["blendmodes_5"] == "host"  # several frames blended: the canvas is a host canvas


@pytest.mark.parametrize("orientation", [3, 6])
def test_orientation_is_a_pass_over_the_resident_planes(backend, orientation):
    """the front-end's header object can be written, so the header's orientation is forced for both decoders"""
    assert _compare(os.path.join(ROOT, "tests", "golden", "samples", "lenna.jxl"), backend, orientation) == "device"


def test_a_trace_listener_still_gets_the_frame_after_the_colour_transforms(backend):
    path = os.path.join(ROOT, "tests", "golden", "samples", "lenna.jxl")
    seen = {}
    for device in (True, False):
        dec = JXLDecoder(path, backend=backend, device_output=device)
        dec.trace = lambda i, stage, planes, fused, d=device: seen.setdefault((d, stage), [np.array(p) for p in planes[:3]])
        im = dec.decode()
        assert dec.stats[-1]["output"] == ("device" if device else "host")
        if device:
            assert "d2h" not in dec.stats[-1]["plane_moves"] and im.onDevice()
    for c in range(3):
        assert_bits_equal(seen[(True, "xyb")][c], seen[(False, "xyb")][c], "xyb cut, plane %d" % c)


def _png_bytes(image):
    out = io.BytesIO()
    PNGWriter(image, deviceSamples=True).write(out)
    return out.getvalue()


def test_an_image_whose_planes_a_later_decode_took_raises(backend):
    path = os.path.join(ROOT, "tests", "golden", "samples", "lenna.jxl")
    _, first = _decode(path, backend, device_output=True)
    _, second = _decode(path, backend, device_output=True)
    from jxlatte_amd import _lib
    with pytest.raises(_lib.IllegalStateException):
        first.getBuffer()
    with pytest.raises(_lib.IllegalStateException):
        PNGWriter(first, deviceSamples=True)
    kept = second.getBuffer()  # downloaded once, then the image's own
    before = _png_bytes(second)  # (from the resident planes: they are still the image's)
    _decode(path, backend, device_output=True)
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(second.getBuffer(), kept))
    # a downloaded image holds its samples: the writer takes the host arrays once the planes are gone, as PFMWriter does
    after = PNGWriter(second, deviceSamples=True)
    assert second.getAlphaIndex() < 0 and after.bus_bytes[0] == sum(a.nbytes for a in kept[:3])  # the three planes went up
    assert _png_bytes(second) == before
