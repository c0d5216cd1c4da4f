"""GPU: the cases of tests/jxl_writer_lossy_cases.py -- Modular frames of an XYB image, with Gaborish, with the EPF under
epf_sigma_for_modular, with do_ycbcr -- through JXLDecoder on the device backend, under the default switches, under each switch set
test_jxl_writer_routes_gpu.py uses and under their union. Every decode is held to the expectation made from the SOURCE arrays under
the same K as the oracle backend on the CPU (jxl_writer_lossy_run.check); no oracle and no second decode in any assertion.

The default switches are also compared at the trace cuts mod / gab / epf / xyb (a trace listener changes the route of
device_frames, so the switch sets are compared in the returned image). Every switch set must DECLINE these frames with the right
reason -- stats say which -- except that an unfiltered integer RGB frame is still the lossless frame the sets accept.

The XYB + alpha case is also packed: PNGWriter(deviceSamples=True) and toTensor against numpy packing of the expected planes."""
import numpy as np
import pytest
import torch

import jxl_writer_cases as WC
import jxl_writer_lossy_cases as C
import jxl_writer_lossy_run as RUN
from jxlatte_amd.decoder import PNGWriter
from test_device_frames_gpu import CountingBackend
from test_jxl_writer_cpu import png_of

pytestmark = pytest.mark.gpu
HALVES = {"xyb sizes": [n for n in C.NAMES if n.startswith("xyb_") and n.split("_")[1][0].isdigit() and "copied" not in n],
          "the others": [n for n in C.NAMES if not (n.startswith("xyb_") and n.split("_")[1][0].isdigit() and "copied" not in n)]}


@pytest.fixture(scope="module")
def backend(ctx):
    return CountingBackend(ctx)


def refusal(name):
    """what _int_rgb_planes_rule must answer for the frame: the reason, or None for a frame the plane-set routes accept"""
    im = C.image(name)
    hf = C.header_fields(im)
    if hf["gab"] or hf["epf_iters"] > 0 or hf["do_ycbcr"]:
        return "a restoration filter or YCbCr"
    if hf["xyb_encoded"]:
        return "an XYB image"
    if im.get("grey", False):
        return "colour planes that are not three int32 planes"
    return None


def check_route(name, config, stats):
    """the switch set declined the frame for the right reason (or took the lossless RGB frame)"""
    st, why = stats[0], refusal(name)
    switches = WC.CONFIGS[config]
    grey = C.image(name).get("grey", False)
    if switches.get("device_image"):
        assert st.get("image") == ("device set (modular frame)" if why is None else "host: " + why), (name, config, st)
        if why is None:
            return
    else:
        assert st["image"] == "host: device_image is off", (name, config, st)
    direct = bool(switches.get("device_output")) and not grey
    if switches.get("device_frames"):
        if direct:
            want = "host: device_output's direct path"
        else:  # (a one-colour image lands its canvas in _canvas_route, after the first frame's rule has spoken)
            want = "device set (modular)" if why is None else "host: " + why
        assert st["frame"] == want, (name, config, st)
    else:
        assert st["frame"] == "host: device_frames is off", (name, config, st)
    if switches.get("device_canvas") and not direct:
        assert st["canvas"] == ("landed: one-colour image" if grey else "device"), (name, config, st)
    else:
        assert st["canvas"] == "host", (name, config, st)


@pytest.mark.parametrize("half", list(HALVES))
def test_default_switches_at_every_cut(backend, half):
    for name in HALVES[half]:
        out = RUN.decode(C.encoded(name), backend)
        try:
            assert RUN.fields_differ(name, out) is None, name
            RUN.check(name, out, name + " on the device")
        finally:
            out["close"]()


@pytest.mark.parametrize("config", list(WC.CONFIGS))
@pytest.mark.parametrize("half", list(HALVES))
def test_every_switch_set_declines_and_decodes(backend, half, config):
    for name in HALVES[half]:
        out = RUN.decode(C.encoded(name), backend, trace=False, **WC.CONFIGS[config])
        try:
            check_route(name, config, out["stats"])
            RUN.check(name, out, "%s under %s" % (name, config), cuts=False)
        finally:
            out["close"]()


def test_a_wrong_expectation_is_seen(backend):
    """the comparison discriminates on the device as it does on the CPU: Cb and Cr exchanged, the grey image's plane 0"""
    for name, mut in (("ycbcr_13x21_gab1_epf2", "cb_cr_exchanged"), ("grey_tagged_xyb_9x11_gab1_epf2", "grey_plane_0"), ("xyb_5x3_gab1_epf2", "padded_to_8")):
        out = RUN.decode(C.encoded(name), backend, trace=False)
        try:
            assert max(RUN.image_ratios(name, out["planes"], C.model(name, mut))) >= 100 * C.bound(name, "xyb"), (name, mut)
        finally:
            out["close"]()


@pytest.mark.parametrize("config", ["default", "canvas", "output", "all"])
def test_packed_samples_of_the_alpha_case(backend, config):
    """PNGWriter(deviceSamples=True) and toTensor(uint8) inside numpy packing of the expected planes at both ends of their bound,
    toTensor(float32) within the planes' own K; the alpha samples are the source's integers"""
    name = "xyb_alpha_13x21_gab1_epf2"
    im = C.image(name)
    h, w = im["height"], im["width"]
    out = RUN.decode(C.encoded(name), backend, trace=False, **WC.CONFIGS[config])
    try:
        image, ends, m = out["image"], C.packed_rgba(name), C.model(name)
        wr = PNGWriter(image, deviceSamples=True)
        got = png_of(wr).astype(np.int64)
        lo, hi = ends("srgb")
        assert wr.bitDepth == 8 and got.shape == lo.shape == (h, w, 4), config
        assert ((lo <= got) & (got <= hi)).all(), (config, "PNG", int(((got < lo) | (got > hi)).sum()))
        assert np.array_equal(got[..., 3], np.asarray(im["frames"][0]["planes"][3])), config
        assert (lo != hi).mean() < 0.02  # the ends agree nearly everywhere: the packing is pinned
        lo, hi = ends("linear")
        model3 = (np.stack([p[0] for p in m["image"][:3]]), np.stack([p[1] for p in m["image"][:3]]))
        for layout in ("CHW", "HWC"):
            t = image.toTensor(torch.float32, layout=layout, target="as-is").cpu().numpy()
            t = t if layout == "CHW" else np.moveaxis(t, -1, 0)
            r = C.ratio(t, model3)
            print("%s tensor float32 %s: ratio %.3f of K = %d" % (config, layout, r, C.bound(name, "xyb")))
            assert t.dtype == np.float32 and r <= C.bound(name, "xyb"), (config, layout, r)
            t = image.toTensor(torch.uint8, layout=layout, target="as-is").cpu().numpy().astype(np.int64)
            t = t if layout == "HWC" else np.moveaxis(t, 0, -1)
            assert t.shape == (h, w, 3) and ((lo[..., :3] <= t) & (t <= hi[..., :3])).all(), (config, layout, "tensor uint8")
    finally:
        out["close"]()
