"""JXLImage.toTensor(size=, box=) on decoded bitstreams: every committed sample, from each home its image can have -- host arrays
(the default decoder), resident planes (device_output) and a device plane set (every device switch on). Each home's tensor equals,
bit for bit, the stage entry on the host planes of the default decode; nothing comes down; two samples of different sizes fill one
batch through out=batch[i]."""
import json
import os

import numpy as np
import pytest
import torch

from jxlatte_amd import host
from jxlatte_amd.decoder import DeviceBackend, JXLDecoder

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = dict(sparse_coeffs=True, device_splines=True, device_patches=True, device_output=True, device_canvas=True, device_palette=True,
           device_image=True, device_frames=True)  # tests/golden/make_decode_routes.py: CONFIGS["all"]
with open(os.path.join(ROOT, "tests", "golden", "decode_routes.json")) as _f:
    NAMES = sorted(json.load(_f)["device"]["samples"])
SIZE = (32, 32)


@pytest.fixture(scope="module")
def backend(ctx):
    be = DeviceBackend.__new__(DeviceBackend)
    be.host, be.ctx, be.palette_log = host, ctx, []
    return be


def _last_image(name, backend, **switches):
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
    if t.dtype == torch.uint8:
        return t.cpu().numpy()
    if t.dtype == torch.float32:
        return t.cpu().numpy().view(np.uint32)
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


def _calls(im):
    """the calls of the test on one image: (what, keywords)"""
    h, w = im.getHeight(), im.getWidth()
    box = (w // 4, h // 4, max(1, w // 2), max(1, h // 2))
    alpha = "append" if im.hasAlpha() else "drop"
    return [("size f32", dict(dtype=torch.float32, layout="CHW", size=SIZE)),
            ("size u8 hwc box filter", dict(dtype=torch.uint8, layout="HWC", size=SIZE, resample="box", alpha=alpha)),
            ("boxed f16 linear", dict(dtype=torch.float16, layout="CHW", target="linear", size=(24, 40), box=box, alpha=alpha)),
            ("crop bf16", dict(dtype=torch.bfloat16, layout="HWC", box=box))]


def _tensors(name, backend, **switches):
    im, dec = _last_image(name, backend, **switches)
    try:
        home = im._home(im.getColorChannelCount(), True)
        out = {}
        for what, kw in _calls(im):
            t = im.toTensor(**kw)
            assert t.device == torch.device("cuda:%d" % backend.ctx.device) and t.is_contiguous()
            assert im.tensor_bus_bytes[1] == 0, "nothing comes down"
            if home == "set":
                assert im.tensor_bus_bytes == (0, 0)
            out[what] = (tuple(t.shape), _bits(t))
        return home, out
    finally:
        im.close()
        dec.close()


@pytest.mark.parametrize("name", NAMES)
def test_to_tensor_resized_from_every_home(backend, name):
    home, exp = _tensors(name, backend)
    assert home == "host", "the default decoder's planes are host arrays: toTensor is the stage entry on them"
    seen = {home}
    for switches in (dict(device_output=True), ALL):
        other, got = _tensors(name, backend, **switches)
        seen.add(other)
        for what in exp:
            assert got[what][0] == exp[what][0], (name, other, what)
            same = got[what][1] == exp[what][1]
            if exp[what][1].dtype == np.uint32:  # NaNs as one value
                f = lambda a: np.isnan(a.view(np.float32))  # noqa: E731
                same = same | (f(got[what][1]) & f(exp[what][1]))
            assert same.all(), "%s from %s: %s: %d elements differ" % (name, other, what, int((~same).sum()))
    assert seen <= {"host", "resident", "set"}


def test_two_samples_of_different_sizes_fill_one_batch(backend):
    dev = torch.device("cuda:%d" % backend.ctx.device)
    batch = torch.full((3, 3, 32, 32), 7.0, dtype=torch.float32, device=dev)
    used = []
    for name in NAMES:
        im, dec = _last_image(name, backend, **ALL)
        try:
            shape = (im.getHeight(), im.getWidth())
            if im.getColorChannelCount() != 3 or shape in [u[1] for u in used]:
                continue
            alone = im.toTensor(size=SIZE)
            r = im.toTensor(size=SIZE, out=batch[len(used)])
            assert r.data_ptr() == batch[len(used)].data_ptr() and torch.equal(_as_int(r), _as_int(alone))
            used.append((name, shape))
        finally:
            im.close()
            dec.close()
        if len(used) == 2:
            break
    assert len(used) == 2 and used[0][1] != used[1][1], "two three-channel samples of different sizes"
    assert bool((batch[2] == 7.0).all()), "the neighbour of the filled slices is left alone"


def _as_int(t):
    return t.contiguous().view(torch.int32)
