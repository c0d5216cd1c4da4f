"""decoder.toTensorBatch on decoded bitstreams: the committed samples, grouped by channel count, from host arrays (the default
decoder) and from device plane sets (device_image=True) on one shared backend. The batch equals torch.stack of the per-image
JXLImage.toTensor(size=...) tensors bit for bit; from sets nothing crosses the bus; out= fills a slice of a larger batch; images
of two backends are refused."""
import json
import os

import numpy as np
import pytest
import torch

from jxlatte_amd import host
from jxlatte_amd.decoder import DeviceBackend, JXLDecoder, toTensorBatch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "decode_routes.json")) as _f:
    NAMES = sorted(json.load(_f)["device"]["samples"])
SIZES = [(16, 24), (7, 5)]
OUTPUTS = [(torch.uint8, "HWC"), (torch.float16, "CHW")]


def _backend(ctx):
    be = DeviceBackend.__new__(DeviceBackend)
    be.host, be.ctx, be.palette_log = host, ctx, []
    return be


@pytest.fixture(scope="module")
def backend(ctx):
    return _backend(ctx)


def _last_image(name, backend, **switches):
    dec = JXLDecoder(os.path.join(ROOT, "tests", "golden", "samples", name + ".jxl"), backend=backend, **switches)
    last = None
    while True:
        im = dec.decode()
        if im is None:
            dec.close()
            return last
        if last is not None:
            last.close()
        last = im


@pytest.fixture(scope="module")
def decoded(backend):
    """every sample's last image, decoded once per home and kept (a set stays the image's own until close)"""
    images = {"host": [_last_image(n, backend) for n in NAMES], "set": [_last_image(n, backend, device_image=True) for n in NAMES]}
    yield images
    for group in images.values():
        for im in group:
            im.close()


def _bits(t):
    return t.cpu().numpy() if t.dtype == torch.uint8 else t.view(torch.int16).cpu().numpy().view(np.uint16)


def _groups(images, alpha="drop"):
    """the images by the channel count their toTensor plan gives (the tensor's shape tells)"""
    groups = {}
    for im in images:
        groups.setdefault(int(im.toTensor(size=(8, 8), alpha=alpha).shape[0]), []).append(im)
    return groups


@pytest.mark.parametrize("home", ["host", "set"])
def test_batch_equals_the_stack_of_per_image_tensors(decoded, home):
    images = decoded[home]
    groups = _groups(images)
    assert sum(len(g) for g in groups.values()) == len(NAMES) and max(len(g) for g in groups.values()) >= 2
    on_set = 0
    for size in SIZES:
        for dtype, layout in OUTPUTS:
            for channels, group in groups.items():
                exp = torch.stack([im.toTensor(dtype=dtype, layout=layout, size=size) for im in group])
                single_bus = [im.tensor_bus_bytes for im in group]
                got = toTensorBatch(group, size, dtype=dtype, layout=layout)
                n = len(group)
                assert tuple(got.shape) == ((n, channels) + size if layout == "CHW" else (n,) + size + (channels,)) and got.dtype == dtype
                assert got.is_contiguous() and got.device == exp.device
                same = _bits(got) == _bits(exp)
                assert same.all(), "%s %s %s %s: %d elements differ" % (home, size, dtype, layout, int((~same).sum()))
                assert [im.tensor_bus_bytes for im in group] == single_bus, "each image's traffic is what toTensor counts for it"
                assert got.bus_bytes == (sum(b[0] for b in single_bus), 0)
                for im in group:
                    if im._home(im.getColorChannelCount(), True) == "set":
                        assert im.tensor_bus_bytes == (0, 0)
                        on_set += 1
                if all(im._home(im.getColorChannelCount(), True) == "set" for im in group):
                    assert got.bus_bytes == (0, 0)
    assert (on_set > 0) == (home == "set")


def test_boxes_and_filters_per_batch(decoded):
    group = max(_groups(decoded["set"]).values(), key=len)
    boxes = [None if k % 2 else (im.getWidth() // 4, im.getHeight() // 4, max(1, im.getWidth() // 2), max(1, im.getHeight() // 2)) for k, im in enumerate(group)]
    exp = torch.stack([im.toTensor(dtype=torch.float16, target="linear", size=(7, 5), box=bx, resample="box") for im, bx in zip(group, boxes)])
    got = toTensorBatch(group, (7, 5), boxes=boxes, dtype=torch.float16, target="linear", resample="box")
    assert np.array_equal(_bits(got), _bits(exp))


def test_out_fills_a_slice_of_a_larger_batch(decoded):
    group = max(_groups(decoded["host"]).values(), key=len)
    n, c = len(group), int(group[0].toTensor(size=(8, 8)).shape[0])
    big = torch.full((n + 3, 16, 24, c), 77, dtype=torch.uint8, device=group[0].toTensor(size=(8, 8)).device)
    exp = torch.stack([im.toTensor(dtype=torch.uint8, layout="HWC", size=(16, 24)) for im in group])
    r = toTensorBatch(group, (16, 24), dtype=torch.uint8, layout="HWC", out=big[2:2 + n])
    assert r.data_ptr() == big[2].data_ptr() and torch.equal(big[2:2 + n], exp)
    assert bool((big[:2] == 77).all()) and bool((big[2 + n:] == 77).all()), "the neighbours of the filled slice are left alone"
    with pytest.raises(ValueError):
        toTensorBatch(group, (16, 24), dtype=torch.uint8, layout="HWC", out=big[2:3 + n])


def test_images_of_two_backends_are_refused(ctx, decoded):
    other = _last_image(NAMES[0], _backend(ctx))
    try:
        with pytest.raises(ValueError, match="different backends"):
            toTensorBatch([decoded["host"][0], other], (7, 5))
        assert toTensorBatch([other], (7, 5)).shape[0] == 1
    finally:
        other.close()
