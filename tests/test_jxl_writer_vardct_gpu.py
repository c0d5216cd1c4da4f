"""GPU: the cases of tests/jxl_writer_vardct_cases.py through JXLDecoder on the device backend. Every switch set a VarDCT frame
reaches -- the default switches, sparse_coeffs, and the opt-in sets that keep the frame's planes resident (device_output,
device_canvas, and both with the sparse feed) -- is held to the float64 models of the SOURCE under the K of
jxl_writer_vardct_run.bound, the same as the oracle backend on the CPU; no oracle and no second decode in any assertion.

Default and sparse_coeffs are compared at the cut points idct / gab / epf (stage-masked runs of the frame's own vardct call) and after
the colour transform; the resident sets after the colour transform, where the fused inverse XYB has run. The unfused inverse XYB is
the backend's stage entry on the planes of the "epf" cut.

The cut after the colour transform of a frame with a tail (upsampling, noise, a custom opsin matrix, YCbCr) is held to
jxl_writer_vardct_cases.expected_image, and the stats say where that tail ran: the colour planes of a frame that is upsampled or has
noise are resident from the restoration kernel's float sink to the end of the tail and cross the bus once (default switches) or not
at all (the resident sets). The alpha cases are also packed: PNGWriter(deviceSamples=True) and toTensor against numpy packing of
the expected planes (jxl_writer_vardct_run.sample_bounds)."""
import numpy as np
import pytest
import torch

import jxl_writer_vardct as V
import jxl_writer_vardct_cases as C
import jxl_writer_vardct_run as R
import vardct_ref64 as M
from jxlatte_amd import host
from jxlatte_amd.decoder import DeviceBackend, PNGWriter
from test_jxl_writer_cpu import png_of

pytestmark = pytest.mark.gpu
NAMES = sorted(C.CASES)
CUT_SETS = (("default", {}), ("sparse_coeffs", dict(sparse_coeffs=True)))
RESIDENT_SETS = (("device_output", dict(device_output=True)), ("device_canvas", dict(device_canvas=True)),
                 ("device_output + sparse_coeffs", dict(device_output=True, sparse_coeffs=True)),
                 ("device_canvas + device_output + sparse_coeffs", dict(device_canvas=True, device_output=True, sparse_coeffs=True)))


class Backend(DeviceBackend):
    """the device backend on the session's context"""

    def __init__(self, ctx):
        self.host, self.ctx = host, ctx
        self.palette_log = []


@pytest.fixture(scope="module")
def backend(ctx):
    return Backend(ctx)


def hold(name, what, got, stage):
    r, k = R.ratio(got, name, stage), R.bound(name, stage)
    print("%s, %s, stages %d: needs K = %.2f of %d" % (name, what, stage, r, k))
    assert r <= k, (name, what, stage, r, k)


def hold_extras(name, what, image):
    """the image's extra channels: the source cast to float bit for bit, or -- upsampled -- the model's within K_UPSAMPLE"""
    planes = image.getBuffer()
    for i, (x, a) in enumerate(C.expected_extras(name)):
        got = np.asarray(planes[3 + i])
        assert got.dtype == np.float32 and got.shape == x.shape, (name, what, i)
        if a is None:
            assert np.array_equal(got.view(np.uint32), np.asarray(x, np.float32).view(np.uint32)), (name, what, i)
        else:
            r = M.error_ratio(got, x, a)
            print("%s, %s, extra channel %d: needs K = %.2f of %d" % (name, what, i, r, R.K_UPSAMPLE))
            assert r <= R.K_UPSAMPLE, (name, what, i, r)


def tail_on_device(src):
    """the frames whose colour planes stay on the device between decodeFrame and the colour transform under every switch set: those
    with a stage in between"""
    return src.get("upsampling", 1) > 1 or src.get("noise") is not None


def is_whole_image(src):
    """device_output hands out the frame's own resident planes when the upsampled frame is the image, to the pixel"""
    return V.image_size(src) == (src["height"] * src.get("upsampling", 1), src["width"] * src.get("upsampling", 1))


@pytest.mark.parametrize("name", NAMES)
def test_device_decode_is_the_model(name, backend):
    src, final = C.source(name), R.final_stage(name)
    for what, switches in CUT_SETS:
        out = R.decode(C.encoded(name), backend, **switches)
        for cut, stage, _ in R.CUTS:
            hold(name, what + " " + cut, out[cut], stage)
        hold(name, what + " after the colour transform", out["xyb"], final)
        if final == R.TAIL:
            st = out["stats"][-1]
            print("%s, %s: %r" % (name, what, {k: st.get(k) for k in ("plane_moves", "output", "canvas")}))
            hold(name, what + " image", np.stack([np.asarray(b) for b in out["image"].getBuffer()[:3]]), final)
            hold_extras(name, what, out["image"])
            if tail_on_device(src):  # resident from the float sink through the tail; one way down, at its end
                assert st["plane_moves"] == ["d2h"], (name, what, st)
        if what == "default" and final == R.XYB:  # the unfused inverse XYB: the stage entry on the planes of the last cut
            p = C.params_of(src)
            planes = np.ascontiguousarray(out["epf"][:, :src["height"], :src["width"]])
            got = backend.xyb(planes, np.array(p.opsin_matrix, np.float32), np.array(p.opsin_bias, np.float32),
                              np.array(p.cbrt_opsin_bias, np.float32), float(p.intensity_target))
            hold(name, "unfused inverse XYB", np.asarray(got), final)
    for what, switches in RESIDENT_SETS:
        out = R.decode(C.encoded(name), backend, cuts=False, **switches)
        hold(name, what, out["xyb"], final)
        st = out["stats"][-1]
        if final == R.TAIL:
            print("%s, %s: %r" % (name, what, {k: st.get(k) for k in ("plane_moves", "output", "canvas")}))
            # the colours never came down for a stage of the tail: the only copy is this test's own trace listener's
            direct = "device_output" in what and is_whole_image(src)
            if direct or "device_canvas" in what:
                assert st["plane_moves"] == ["trace"], (name, what, st)
            if "device_canvas" in what and not direct:
                assert st["canvas"] == "device", (name, what, st)
            hold_extras(name, what, out["image"])
        if "device_output" in what and (final != R.TAIL or is_whole_image(src) or "device_canvas" in what):
            # the image's planes came from the resident planes (JXLImage.resident), not from a host frame
            assert st["output"] == "device", (name, what, st)
            hold(name, what + " image", np.stack([np.asarray(b) for b in out["image"].getBuffer()[:3]]), final)


@pytest.mark.parametrize("name", ("alpha_40x40", "alpha_264x264", "alpha_up2"))
def test_packed_samples_of_an_alpha_case(name, backend):
    """the image of an alpha case through the device exits, from host planes (default switches) and from resident ones
    (device_output): PNGWriter(deviceSamples=True) and toTensor(uint8) inside numpy packing of the expected planes, toTensor(float32)
    within the planes' own K; alpha that was not upsampled comes out as the source's integers"""
    src, final = C.source(name), R.final_stage(name)
    ih, iw = V.image_size(src)
    for what, switches in (("default", {}), ("device_output", dict(device_output=True))):
        out = R.decode(C.encoded(name), backend, cuts=False, **switches)
        image = out["image"]
        w = PNGWriter(image, deviceSamples=True)
        got = png_of(w).astype(np.int64)
        lo, hi = R.sample_bounds(name, "srgb")
        assert w.bitDepth == 8 and got.shape == lo.shape == (ih, iw, 4), (name, what)
        assert ((lo <= got) & (got <= hi)).all(), (name, what, "PNG", int(((got < lo) | (got > hi)).sum()))
        if name != "alpha_up2":
            assert np.array_equal(got[..., 3], np.asarray(src["extra"][0]["plane"])), (name, what)
        lo, hi = R.sample_bounds(name, "linear")
        for layout in ("CHW", "HWC"):
            t = image.toTensor(torch.float32, layout=layout, target="as-is").cpu().numpy()
            t = t if layout == "CHW" else np.moveaxis(t, -1, 0)
            assert t.shape == (3, ih, iw), (name, what, layout)
            hold(name, "%s tensor float32 %s" % (what, layout), t, final)
            t = image.toTensor(torch.uint8, layout=layout, target="as-is").cpu().numpy().astype(np.int64)
            t = t if layout == "HWC" else np.moveaxis(t, 0, -1)
            assert t.shape == (ih, iw, 3) and ((lo[..., :3] <= t) & (t <= hi[..., :3])).all(), (name, what, layout, "tensor uint8")
        if what == "device_output":
            assert out["stats"][-1]["output"] == "device", (name, out["stats"][-1])
