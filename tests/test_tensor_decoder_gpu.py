"""JXLImage.toTensor on decoded bitstreams: every committed sample whose image, with every device switch on (the `all` route of
tests/golden/decode_routes.json), ends as a device plane set or as resident planes, and the one that ends on host arrays. The
uint8 tensor equals the samples PNGWriter(deviceSamples=True) takes from a second, identical decode; the linear float32 tensor equals
JXLImage.transform(device=True) of a default decode, whose planes are host arrays; a live set moves nothing over the bus; a slice
of a batch is filled in place and its neighbours are left alone."""
import json
import os

import numpy as np
import pytest
import torch

import tensor_ref as ref
from conftest import assert_bits_equal
from jxlatte_amd import host
from jxlatte_amd.decoder import PRI_SRGB, TF_LINEAR, WP_D65, DeviceBackend, JXLDecoder, PNGWriter

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = dict(sparse_coeffs=True, device_splines=True, device_patches=True, device_output=True, device_canvas=True, device_palette=True,
           device_image=True, device_frames=True)  # tests/golden/make_decode_routes.py: CONFIGS["all"]
with open(os.path.join(ROOT, "tests", "golden", "decode_routes.json")) as _f:
    _ROUTES = json.load(_f)["device"]["samples"]


def _home(name):
    last = _ROUTES[name]["all"]["stats"][-1]
    return "set" if last["image"].startswith("device set") else "resident" if last["output"] == "device" else "host"


ON_DEVICE = sorted(n for n in _ROUTES if _home(n) != "host")
ON_HOST = sorted(n for n in _ROUTES if _home(n) == "host")[:1]


@pytest.fixture(scope="module")
def backend(ctx):
    be = DeviceBackend.__new__(DeviceBackend)
    be.host, be.ctx, be.palette_log = host, ctx, []
    return be


def _last_image(name, backend, **switches):
    """the sample decoded to the end: its last image (the earlier ones released), and the decoder"""
    dec = JXLDecoder(os.path.join(ROOT, "tests", "golden", "samples", name + ".jxl"), backend=backend, **switches)
    last = None
    while True:
        im = dec.decode()
        if im is None:
            return last, dec
        if last is not None:
            last.close()
        last = im


def _bits(t):
    """a tensor's elements as numpy bit patterns"""
    if t.dtype == torch.uint8:
        return t.cpu().numpy()
    if t.dtype == torch.float32:
        return t.cpu().numpy().view(np.uint32)
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


@pytest.mark.parametrize("name", ON_DEVICE + ON_HOST)
def test_to_tensor_on_a_decoded_sample(backend, name):
    home = _home(name)
    im, dec = _last_image(name, backend, **ALL)
    im2 = dec2 = None
    try:
        assert im._home(im.getColorChannelCount(), True) == home, "the record's route"
        has_alpha = im.hasAlpha()
        colors = im.getColorChannelCount()
        # 1. uint8, HWC: the PNG's samples
        t = im.toTensor(torch.uint8, "HWC", alpha="append" if has_alpha else "drop")
        assert t.device == torch.device("cuda:%d" % backend.ctx.device) and t.is_contiguous()
        if home == "set":
            assert im.tensor_bus_bytes == (0, 0) and im.setLive()
        # 2. a slice of a batch is filled in place; its neighbours stay
        batch = torch.full((3,) + tuple(t.shape), 0xA5, dtype=torch.uint8, device=t.device)
        r = im.toTensor(torch.uint8, "HWC", alpha="append" if has_alpha else "drop", out=batch[1])
        assert r.data_ptr() == batch[1].data_ptr() and torch.equal(batch[1], t)
        assert bool((batch[0] == 0xA5).all()) and bool((batch[2] == 0xA5).all())
        # 3. float32, CHW, linear sRGB: JXLImage.transform of a decode whose planes are on the host
        lin = im.toTensor(torch.float32, "CHW", target="linear")
        half = im.toTensor(torch.bfloat16, "CHW", target="linear")
        if home == "set":
            assert im.tensor_bus_bytes == (0, 0)
        # (1.) the second, identical decode -- after the tensors: one context holds one set of resident planes, and this decode takes them
        im2, dec2 = _last_image(name, backend, **ALL)
        w = PNGWriter(im2, bitDepth=8, deviceSamples=True)
        assert w.bus_bytes is not None, "the one-pass writer took the image"
        assert t.shape == w.samples.shape and np.array_equal(_bits(t), w.samples), name
        plain, dec3 = _last_image(name, backend)
        try:
            assert not plain.onDevice()
            exp_im = plain if plain.has_icc else plain.transform(PRI_SRGB, WP_D65, TF_LINEAR, device=True)
            n_out = exp_im.getColorChannelCount()
            exp = [exp_im._as_float(c) for c in range(n_out)]
            if plain.isAlphaPremultiplied() and has_alpha:
                a = plain.getColorChannelCount() + plain.getAlphaIndex()
                exp = ref.unpremultiply(exp, plain._as_float(a))
            assert lin.shape == (n_out, im.getHeight(), im.getWidth())
            assert_bits_equal(lin.cpu().numpy(), np.stack(exp), name + ": linear float32", any_nan=True)
            assert np.array_equal(_bits(half), np.stack(ref.convert(list(lin.cpu().numpy()), "bfloat16"))), name + ": bfloat16"
        finally:
            plain.close()
            dec3.close()
        assert colors in (1, 3)
    finally:
        for x in (im, im2):
            if x is not None:
                x.close()
        for d in (dec, dec2):
            if d is not None:
                d.close()
