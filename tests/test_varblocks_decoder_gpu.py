"""JXLDecoder(draw_varblocks=True) on committed bitstreams: the two smallest VarDCT samples are decoded once without the switch,
the model of tests/varblocks_ref.py is applied to those planes with the block list read from the front-end, and the switch must
give exactly those planes on the default path (the stage entry on host planes), with device_output (the resident planes, and
PNGWriter(deviceSamples=True) packs them where they are) and with device_canvas. A Modular sample is left alone. The command line
takes --draw-varblocks."""
import io
import os
import struct

import numpy as np
import pytest

import varblocks_ref as ref
from conftest import assert_bits_equal
from jxlatte_amd import frontend
from jxlatte_amd.decoder import DeviceBackend, JXLDecoder, JXLImage, PNGWriter

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAMPLES = os.path.join(ROOT, "tests", "golden", "samples")
VARDCT = [os.path.join(SAMPLES, "white.jxl"), os.path.join(SAMPLES, "lenna.jxl")]  # 320 x 240 and 512 x 512, one frame each
MODULAR = os.path.join(SAMPLES, "quilt.jxl")


@pytest.fixture(scope="module")
def backend(ctx):
    from jxlatte_amd import host
    be = DeviceBackend.__new__(DeviceBackend)
    be.host, be.ctx = host, ctx
    return be


def _blocks_from_the_front_end(path, backend):
    """(cy, cx, type) of the first frame as Frame.drawVarblocks walks it: LF group by LF group, block by block"""
    fe = frontend.Frontend(open(path, "rb").read())
    fr = fe.next_frame(backend.squeeze, backend.rct)
    rows = []
    for i in range(fr.num_lf_groups):
        g = fe.lfgroup(i)
        oy, ox = (i // fr.lf_group_cols) << 8, (i % fr.lf_group_cols) << 8
        for y, x in g["block_yx"]:
            rows.append((int(y) + oy, int(x) + ox, int(g["dct_select"][y, x])))
    fe.close()
    return rows


@pytest.fixture(scope="module")
def expected(backend):
    """per VarDCT sample: the default decode (switch off), and the model's drawing on its planes -- computed once"""
    out = {}
    for path in VARDCT:
        dec = JXLDecoder(path, backend=backend)
        im = dec.decode()
        assert dec.info.orientation == 1 and isinstance(dec.stats[-1]["varblocks"], dict)  # (without the switch: the type histogram)
        planes = [np.array(p, copy=True) for p in im.getBuffer(False)]
        blocks = _blocks_from_the_front_end(path, backend)
        assert sum(dec.stats[-1]["varblocks"].values()) == len(blocks) > 0
        # the condition of tests/test_varblocks_gpu.py for these samples: no cube root near a midpoint between two floats
        root = ref.light_root(*planes[:3]).reshape(-1)
        root = root[np.isfinite(root) & (root != 0)]
        f = root.astype(np.float32)
        lo = np.where(f.astype(np.float64) <= root, f, np.nextafter(f, np.float32(-np.inf)))
        mid = (lo.astype(np.float64) + np.nextafter(lo, np.float32(np.inf)).astype(np.float64)) * 0.5
        assert (np.abs(root - mid) / np.spacing(np.abs(root))).min() >= 4
        drawn = ref.draw(planes[:3], blocks)
        assert not all(np.array_equal(a, b) for a, b in zip(drawn, planes[:3]))
        out[path] = (planes, drawn, dec.info)
    return out


def _same(got, drawn, what):
    for c in range(3):
        assert_bits_equal(np.asarray(got[c]), drawn[c], "%s plane %d" % (what, c), any_nan=True)


@pytest.mark.parametrize("path", VARDCT, ids=["white", "lenna"])
def test_default_path_draws_through_the_stage_entry(backend, expected, path):
    dec = JXLDecoder(path, backend=backend, draw_varblocks=True)
    im = dec.decode()
    assert dec.stats[-1]["varblocks"] == "host planes" and dec.stats[-1]["output"] == "host"
    assert isinstance(dec.stats[-1]["varblock_types"], dict)
    _same(im.getBuffer(False), expected[path][1], "default")


@pytest.mark.parametrize("path", VARDCT, ids=["white", "lenna"])
def test_device_output_draws_on_the_resident_planes(backend, expected, path):
    planes, drawn, info = expected[path]
    dec = JXLDecoder(path, backend=backend, device_output=True, draw_varblocks=True)
    im = dec.decode()
    assert dec.stats[-1]["varblocks"] == "device planes" and dec.stats[-1]["output"] == "device" and im.onDevice()
    assert "d2h" not in dec.stats[-1]["plane_moves"]
    w = PNGWriter(im, deviceSamples=True)  # while the planes are still on the device
    model_im = JXLImage([np.array(p, copy=True) for p in drawn] + planes[3:], info, backend)
    r = PNGWriter(model_im, deviceColor=True)
    assert (w.bitDepth, w.colorMode, w.width, w.height) == (r.bitDepth, r.colorMode, r.width, r.height)
    assert w.samples.shape == r.samples.shape and np.array_equal(w.samples, r.samples)
    _same(im.getBuffer(False), drawn, "device_output")


@pytest.mark.parametrize("path", VARDCT, ids=["white", "lenna"])
def test_device_canvas_draws_before_the_blend(backend, expected, path):
    dec = JXLDecoder(path, backend=backend, device_canvas=True, draw_varblocks=True)
    im = dec.decode()
    assert dec.stats[-1]["varblocks"] == "device planes" and dec.stats[-1]["canvas"] == "device"
    _same(im.getBuffer(False), expected[path][1], "device_canvas")
    dec.close()


def test_a_modular_frame_is_left_alone(backend):
    off = JXLDecoder(MODULAR, backend=backend)
    a = off.decode().getBuffer(False)
    for kw in (dict(), dict(device_output=True)):
        on = JXLDecoder(MODULAR, backend=backend, draw_varblocks=True, **kw)
        b = on.decode().getBuffer(False)
        assert all("varblocks" not in st for st in on.stats)
        assert len(a) == len(b) and all(x.dtype == y.dtype and x.tobytes() == y.tobytes() for x, y in zip(a, b))
        on.close()


def _idat(png):
    assert png[:8] == b"\x89PNG\r\n\x1a\n"
    at, data = 8, b""
    while at < len(png):
        n, kind = struct.unpack(">I4s", png[at:at + 8])
        if kind == b"IDAT":
            data += png[at + 8:at + 8 + n]
        at += 12 + n
    return data


def test_cli_flag(backend, tmp_path):
    from jxlatte_amd.__main__ import main
    path = VARDCT[0]
    plain, drawn, drawn_dev = (str(tmp_path / n) for n in ("plain.png", "drawn.png", "drawn_dev.png"))
    assert main([path, plain]) == 0
    assert main([path, drawn, "--draw-varblocks", "--device-color"]) == 0
    assert main([path, drawn_dev, "--draw-varblocks", "--device-png"]) == 0
    files = [open(p, "rb").read() for p in (plain, drawn, drawn_dev)]
    # with the flag off: the file the decoder and the writer give without the switch, as the command line calls them
    im = JXLDecoder(path, backend=backend).decode()
    out = io.BytesIO()
    PNGWriter(im, bitDepth=16 if im.isHDR() else -1, hdr=im.isHDR()).write(out)
    assert files[0] == out.getvalue()
    assert _idat(files[1]) and _idat(files[1]) != _idat(files[0])
    assert _idat(files[2]) == _idat(files[1])  # --device-png gives --device-color's bytes, as for every picture
