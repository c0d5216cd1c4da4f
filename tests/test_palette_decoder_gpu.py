"""JXLDecoder(device_palette=True) on committed bitstreams: patches-lossless.jxl undoes four frame-level palettes in each of its
two frames (one of four channels, then three of one) and must give the planes it gives without the switch, with the four
transforms listed in stats[k]["palette"]; quilt.jxl has no palette, is unchanged and lists none."""
import os

import numpy as np
import pytest

from jxlatte_amd.decoder import DeviceBackend, JXLDecoder

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAMPLES = os.path.join(ROOT, "tests", "golden", "samples")


@pytest.fixture(scope="module")
def backend(ctx):
    from jxlatte_amd import host
    be = DeviceBackend.__new__(DeviceBackend)
    be.host, be.ctx = host, ctx
    return be


def _decode(path, backend, **kw):
    dec = JXLDecoder(path, backend=backend, **kw)
    im = dec.decode()
    return dec, [np.array(p, copy=True) for p in im.getBuffer(False)]


def test_palette_file_gives_the_same_planes_and_lists_its_transforms(backend):
    path = os.path.join(SAMPLES, "patches-lossless.jxl")
    plain, want = _decode(path, backend)
    dec, got = _decode(path, backend, device_palette=True)
    assert len(got) == len(want) and all(a.dtype == b.dtype and np.array_equal(a, b) for a, b in zip(got, want))
    assert len(dec.stats) == len(plain.stats) == 2 and all("palette" not in s for s in plain.stats)
    for s in dec.stats:
        pal = s["palette"]
        assert [p["num_c"] for p in pal] == [4, 1, 1, 1]
        assert all(set(p) == {"num_c", "nb_colors", "delta_pixels", "launches"} for p in pal)
        assert all(p["nb_colors"] > 100 and p["launches"] == 1 and p["delta_pixels"] == 0 for p in pal)
    assert {dec.stats[0]["palette"][0]["nb_colors"], dec.stats[1]["palette"][0]["nb_colors"]} == {326, 335}


def test_file_without_palettes_is_unchanged_and_lists_none(backend):
    path = os.path.join(SAMPLES, "quilt.jxl")
    _, want = _decode(path, backend)
    dec, got = _decode(path, backend, device_palette=True)
    assert len(got) == len(want) and all(a.dtype == b.dtype and np.array_equal(a, b) for a, b in zip(got, want))
    assert [s["palette"] for s in dec.stats] == [[]] * len(dec.stats) and dec.stats


def test_backend_without_palette_is_an_error(backend):
    class NoPalette:
        def __init__(self, be):
            self.squeeze, self.rct = be.squeeze, be.rct
    with pytest.raises(RuntimeError, match="palette"):
        JXLDecoder(os.path.join(SAMPLES, "quilt.jxl"), backend=NoPalette(backend), device_palette=True).decode()
