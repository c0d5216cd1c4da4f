"""JXLDecoder(region=) on the device.

* the window exit: jxl_planes_from_frame_at against a numpy slice of jxl_vardct_read_output, on frame A;
* noise on a window (csrc/k_noise_window.hip): jxl_stage_noise_window and jxl_planes_noise_at bit-equal to jxl_stage_noise_init +
  jxl_stage_noise_add of the whole frame, cropped, on the windows of tests/region_cases.py's frame E; both refuse what the
  validator refuses;
* the decoder on the device backend: the region decode equals the device's full decode with the same switches, cropped, bit for
  bit -- by default, with sparse_coeffs and with device_output, where the image is a resident-planes home, nothing crosses the bus
  for toTensor, and toTensor(size=) of the region is toTensor(size=, box=region) of the full image;
* a frame that does not qualify raises on the device backend too; the CLI's exit code."""
import os

import numpy as np
import pytest
import torch

import region_cases as RC
import test_region_cpu as R
from conftest import assert_bits_equal
from jxlatte_amd import _lib, abi, host
from jxlatte_amd.decoder import DeviceBackend, JXLDecoder, UnsupportedOperationException, feed_frame

pytestmark = pytest.mark.gpu
F = np.float32
SWITCHES = {"default": {}, "sparse_coeffs": dict(sparse_coeffs=True), "device_output": dict(device_output=True)}
NAMES = ("A", "B", "C", "D", "E", "F1", "F2") + R.FILES


@pytest.fixture(scope="module")
def backend():
    b = DeviceBackend(0)
    yield b
    b.close()


# ---- the window exit -----------------------------------------------------------------------------------------------------------------
def test_planes_from_frame_at_is_a_slice_of_the_result(backend):
    dec = JXLDecoder(RC.encoded("A"), backend=backend)
    fr = dec._next_frame()
    p, weights, woffs, lfgroups, groups, _ = dec._vardct_inputs(fr, False)
    hf = feed_frame(host.Frame(backend.ctx, p, weights, woffs), lfgroups, groups(False), False)
    hf.run()
    full = hf.readOutput()
    assert full.shape == (3, 520, 520) and full.dtype == np.float32
    for y0, x0, h, w in ((0, 0, 520, 520), (0, 0, 8, 8), (263, 263, 242, 242), (519, 519, 1, 1), (1, 517, 300, 3), (255, 0, 2, 520)):
        backend.ctx.call("jxl_planes_from_frame_at", y0, x0, h, w)
        rp = host.ResidentPlanes(backend.ctx)
        assert rp.shape == (h, w)
        assert_bits_equal(rp.download(), full[:, y0:y0 + h, x0:x0 + w], "window %s" % ((y0, x0, h, w),))
    backend.ctx.call("jxl_planes_from_frame", 100, 90)  # the (0, 0) case is the old entry
    assert_bits_equal(host.ResidentPlanes(backend.ctx).download(), full[:, :100, :90], "jxl_planes_from_frame")
    for bad in ((-1, 0, 8, 8), (0, -1, 8, 8), (0, 0, 0, 8), (0, 0, 8, 0), (513, 0, 8, 8), (0, 513, 8, 8), (0, 0, 521, 1), (2147483647, 0, 2, 1)):
        with pytest.raises(_lib.JxlError) as e:
            backend.ctx.call("jxl_planes_from_frame_at", *bad)
        assert e.value.status == abi.JXL_ERR_INVALID_ARGUMENT
    assert host.ResidentPlanes(backend.ctx).shape == (100, 90)  # a refused call leaves the planes alone


# ---- noise on a window ---------------------------------------------------------------------------------------------------------------
FRAME_H, FRAME_W, GROUP_DIM = 264, 520, 256
NOISE_LUT = np.array([0, 300, 1023, 640, 900, 120, 0, 512], F) / F(1024)
BCX, BCB = 0.05, 0.9
_noise = {}


def noise_reference(ctx, seed0):
    """(planes before, planes after) of the whole frame through jxl_stage_noise_init + jxl_stage_noise_add, once per seed; the
    planes put the strength's inputs 3 (Y +- X) under 0, between the LUT's segments and over 7"""
    if seed0 not in _noise:
        rng = np.random.default_rng(77)
        planes = np.stack([rng.uniform(-1.5, 1.5, (FRAME_H, FRAME_W)), rng.uniform(-0.5, 2.5, (FRAME_H, FRAME_W)),
                           rng.uniform(0, 1, (FRAME_H, FRAME_W))]).astype(F)
        v = 3 * np.stack([planes[1] + planes[0], planes[1] - planes[0]])
        assert (v < 0).any() and (v >= 7).any() and len(set(np.floor(v[(v >= 0) & (v < 7)]).astype(int).tolist())) == 7
        noise = host.initializeNoise(ctx, FRAME_H, FRAME_W, seed0, GROUP_DIM, 3)
        after = host.synthesizeNoise(ctx, planes, noise, NOISE_LUT, BCX, BCB)
        assert (after.view(np.uint32) != planes.view(np.uint32)).mean() > 0.5
        planes.setflags(write=False)
        after.setflags(write=False)
        _noise[seed0] = (planes, after)
    return _noise[seed0]


@pytest.mark.parametrize("seed0", [1 << 32, (3 << 32) | 2])
@pytest.mark.parametrize("i", range(6))
def test_noise_on_a_window_is_the_frames_noise_cropped(ctx, i, seed0):
    x0, y0, w, h = RC.boxes("E")[i]
    before, after = noise_reference(ctx, seed0)
    crop = np.ascontiguousarray(before[:, y0:y0 + h, x0:x0 + w])
    want = after[:, y0:y0 + h, x0:x0 + w]
    got = host.noiseWindow(ctx, crop, GROUP_DIM, seed0, NOISE_LUT, BCX, BCB, FRAME_H, FRAME_W, y0, x0)
    assert_bits_equal(got, want, "jxl_stage_noise_window %s" % ((x0, y0, w, h),))
    rp = host.ResidentPlanes.upload(ctx, crop)
    rp.noiseAt(GROUP_DIM, seed0, NOISE_LUT, BCX, BCB, FRAME_H, FRAME_W, y0, x0)
    assert rp.shape == (h, w)
    assert_bits_equal(rp.download(), want, "jxl_planes_noise_at %s" % ((x0, y0, w, h),))


def test_noise_with_smaller_groups(ctx):
    """64-pixel groups: a 70 x 150 window then spans 3 x 4 groups, none of them whole"""
    seed0, gd = 5, 64
    before, _ = noise_reference(ctx, 1 << 32)
    after = host.synthesizeNoise(ctx, before, host.initializeNoise(ctx, FRAME_H, FRAME_W, seed0, gd, 3), NOISE_LUT, BCX, BCB)
    y0, x0, h, w = 60, 100, 70, 150
    got = host.noiseWindow(ctx, np.ascontiguousarray(before[:, y0:y0 + h, x0:x0 + w]), gd, seed0, NOISE_LUT, BCX, BCB, FRAME_H, FRAME_W, y0, x0)
    assert_bits_equal(got, after[:, y0:y0 + h, x0:x0 + w], "64-pixel groups")


def test_the_noise_entries_refuse_what_the_validator_refuses(ctx):
    planes = np.zeros((3, 20, 20), F)
    for gd, fh, fw, y0, x0 in ((256, 264, 520, 250, 0), (256, 264, 520, 0, 501), (256, 264, 520, -1, 0), (256, 0, 520, 0, 0), (24, 264, 520, 0, 0),
                               (8, 264, 520, 0, 0), (256, 40000, 40000, 0, 0)):
        with pytest.raises(_lib.JxlError) as e:
            host.noiseWindow(ctx, planes, gd, 1, NOISE_LUT, BCX, BCB, fh, fw, y0, x0)
        assert e.value.status == abi.JXL_ERR_INVALID_ARGUMENT and "noise window" in str(e.value)
        rp = host.ResidentPlanes.upload(ctx, planes)
        with pytest.raises(_lib.JxlError) as e:
            rp.noiseAt(gd, 1, NOISE_LUT, BCX, BCB, fh, fw, y0, x0)
        assert e.value.status == abi.JXL_ERR_INVALID_ARGUMENT and "noise window" in str(e.value)
        assert_bits_equal(rp.download(), planes, "a refused call leaves the planes alone")


# ---- the decoder ---------------------------------------------------------------------------------------------------------------------
_full = {}


def device_full(backend, name, switch):
    """the device's full decode under a switch set, once per file"""
    if (name, switch) not in _full:
        planes = [np.array(p, copy=True) for p in JXLDecoder(R.data_of(name), backend=backend, **SWITCHES[switch]).decode().getBuffer(copy=False)]
        for p in planes:
            p.setflags(write=False)
        _full[name, switch] = planes
    return _full[name, switch]


def boxes_of(name, switch):
    boxes = RC.boxes(name) if name in RC.FRAMES else R.sample_boxes(name)
    return boxes if switch == "default" else boxes[:3]


@pytest.mark.parametrize("switch", sorted(SWITCHES))
@pytest.mark.parametrize("name", NAMES)
def test_device_region_equals_the_device_crop(backend, name, switch):
    full = device_full(backend, name, switch)
    for box in boxes_of(name, switch):
        dec = JXLDecoder(R.data_of(name), backend=backend, region=box, **SWITCHES[switch])
        im = dec.decode()
        st = dec.stats[-1]
        assert st["region"]["box"] == tuple(box) and st["output"] == ("device" if switch == "device_output" else "host")
        assert im.region == tuple(box) and (im.getWidth(), im.getHeight()) == (box[2], box[3])
        if switch == "device_output":
            assert im.onDevice() and im._home(3) == "resident"
            t = im.toTensor()
            assert im.tensor_bus_bytes == (0, 0) and t.is_cuda and tuple(t.shape) == (3, box[3], box[2])
            assert im._buffer[0] is None, "toTensor brought the planes down"
        for c, (a, b) in enumerate(zip(im.getBuffer(copy=False), RC.crop(full, box))):
            assert_bits_equal(a, b, "%s %s %s plane %d" % (name, switch, box, c))
        assert dec.decode() is None


def test_the_device_reads_what_the_cpu_reads(backend):
    for name in ("A", "B", "lenna"):
        for box in boxes_of(name, "default"):
            a = JXLDecoder(R.data_of(name), backend=backend, region=box)
            a.decode()
            b = R.region_decode(name, box)[0]
            assert a.stats[-1]["region"] == b.stats[-1]["region"]


@pytest.mark.parametrize("name", ("A", "E", "bbb"))
def test_the_resident_region_feeds_the_resized_tensor(backend, name):
    """toTensor(size=) of the region is toTensor(size=, box=region) of the full image, both from resident planes"""
    box = boxes_of(name, "device_output")[1]
    full = JXLDecoder(R.data_of(name), backend=backend, device_output=True).decode()
    want = full.toTensor(size=(64, 64), box=box).clone()
    assert full.tensor_bus_bytes == (0, 0)
    im = JXLDecoder(R.data_of(name), backend=backend, device_output=True, region=box).decode()
    got = im.toTensor(size=(64, 64))
    assert im.tensor_bus_bytes == (0, 0) and tuple(got.shape) == (3, 64, 64)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["art", "patches-lossless", "up8_40x40", "s420", "alpha_40x40"])
def test_a_refused_frame_raises_on_the_device_backend_too(backend, name):
    want = R.RULE[name] if name in R.RULE else R.WRITER_RULE[name]
    for kw in SWITCHES.values():
        with pytest.raises(UnsupportedOperationException) as e:
            JXLDecoder(R.data_of(name), backend=backend, region=(0, 0, 4, 4), **kw).decode()
        assert str(e.value) == "region: " + want


def test_the_cli_exit_codes(tmp_path, capsys):
    from jxlatte_amd import __main__ as cli
    out = str(tmp_path / "out.png")
    assert cli.main(["--region=236,100,40,70", "--device-png", os.path.join(R.SAMPLES, "lenna.jxl"), out]) == 0
    with open(out, "rb") as f:
        assert f.read()[16:24] == (40).to_bytes(4, "big") + (70).to_bytes(4, "big")
    assert cli.main(["--region=0,0,8,8", os.path.join(R.SAMPLES, "art.jxl"), out]) == 2
    assert "region: not a VarDCT frame" in capsys.readouterr().err
