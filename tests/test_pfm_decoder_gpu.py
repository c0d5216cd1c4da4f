"""PFMWriter on decoded bitstreams: the smallest VarDCT sample (its one frame is the image, so device_output leaves the planes on
the device and jxl_planes_pfm_samples packs them) and the smallest Modular sample (integer planes on the host, through
jxl_stage_pfm_samples). PFMWriter(deviceSamples=True) on a device_output decode writes the file PFMWriter() writes on a default
decode, byte for byte, and so does the command line with --format=pfm --device-png."""
import io
import os

import pytest

import pfm_ref
from jxlatte_amd.decoder import DeviceBackend, JXLDecoder, PFMWriter

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARDCT = os.path.join(ROOT, "tests", "golden", "samples", "white.jxl")   # 122 bytes, 320 x 240, XYB
MODULAR = os.path.join(ROOT, "tests", "golden", "samples", "quilt.jxl")  # 27 bytes, 1024 x 1024, 8-bit integer planes


@pytest.fixture(scope="module")
def backend(ctx):
    from jxlatte_amd import host
    be = DeviceBackend.__new__(DeviceBackend)
    be.host, be.ctx = host, ctx
    return be


def _file(writer):
    out = io.BytesIO()
    writer.write(out)
    return out.getvalue()


@pytest.fixture(scope="module")
def host_files(backend):
    """the default decode and the default writer, once per sample; the model confirms them"""
    files = {}
    for path in (VARDCT, MODULAR):
        im = JXLDecoder(path, backend=backend).decode()
        files[path] = _file(PFMWriter(im))
        assert files[path] == pfm_ref.pfm(im.getBuffer(False)[:3], [im.getTaggedBitDepth(c) for c in range(3)])
    return files


def test_vardct_sample_stays_on_the_device(backend, host_files):
    dec = JXLDecoder(VARDCT, backend=backend, device_output=True)
    im = dec.decode()
    assert dec.stats[-1]["output"] == "device" and im.onDevice()
    w = PFMWriter(im, deviceSamples=True)
    assert "d2h" not in dec.stats[-1]["plane_moves"]
    payload = 4 * 3 * im.getWidth() * im.getHeight()
    assert w.bus_bytes == (0, payload)
    got = _file(w)
    assert got == host_files[VARDCT] and len(got) == len(pfm_ref.header(3, im.getHeight(), im.getWidth())) + payload


def test_modular_sample_goes_through_the_stage_entry(backend, host_files):
    dec = JXLDecoder(MODULAR, backend=backend, device_output=True)
    im = dec.decode()
    assert dec.stats[-1]["output"] == "host" and not im.onDevice()
    assert all(str(b.dtype) == "int32" for b in im.getBuffer(False)[:3])
    w = PFMWriter(im, deviceSamples=True)
    payload = 4 * 3 * im.getWidth() * im.getHeight()
    assert w.bus_bytes == (payload, payload)
    assert _file(w) == host_files[MODULAR]


def test_an_image_whose_planes_a_later_decode_took_raises(backend):
    from jxlatte_amd import _lib
    first = JXLDecoder(VARDCT, backend=backend, device_output=True).decode()
    JXLDecoder(VARDCT, backend=backend, device_output=True).decode()
    with pytest.raises(_lib.IllegalStateException):
        PFMWriter(first, deviceSamples=True)


@pytest.mark.parametrize("path", [VARDCT, MODULAR], ids=["vardct", "modular"])
def test_cli_writes_the_same_file(host_files, tmp_path, path):
    from jxlatte_amd.__main__ import main
    out = str(tmp_path / "out.bin")
    assert main([path, out, "--format=pfm", "--device-png"]) == 0
    assert open(out, "rb").read() == host_files[path]
    named = str(tmp_path / "OUT.PFM")  # the extension alone selects the format; the host writer
    assert main([path, named]) == 0
    assert open(named, "rb").read() == host_files[path]
