"""GPU: the cases of tests/jxl_writer_vardct_cases.py through JXLDecoder on the device backend. Every switch set a VarDCT frame
reaches -- the default switches, sparse_coeffs, and the opt-in sets that keep the frame's planes resident (device_output,
device_canvas, and both with the sparse feed) -- is held to the float64 models of the SOURCE under the K of
jxl_writer_vardct_run.bound, the same as the oracle backend on the CPU; no oracle and no second decode in any assertion.

Default and sparse_coeffs are compared at the cut points idct / gab / epf (stage-masked runs of the frame's own vardct call) and after
the colour transform; the resident sets after the colour transform, where the fused inverse XYB has run. The unfused inverse XYB is
the backend's stage entry on the planes of the "epf" cut. A YCbCr frame has no modelled colour transform: it is compared at "epf"."""
import numpy as np
import pytest

import jxl_writer_vardct_cases as C
import jxl_writer_vardct_run as R
from jxlatte_amd import host
from jxlatte_amd.decoder import DeviceBackend

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


@pytest.mark.parametrize("name", NAMES)
def test_device_decode_is_the_model(name, backend):
    src, final = C.source(name), R.final_stage(name)
    for what, switches in CUT_SETS:
        out = R.decode(C.encoded(name), backend, **switches)
        for cut, stage, _ in R.CUTS:
            hold(name, what + " " + cut, out[cut], stage)
        if final is not None:
            hold(name, what + " after the colour transform", out["xyb"], final)
        if what == "default" and final == R.XYB:  # the unfused inverse XYB: the stage entry on the planes of the last cut
            p = C.params_of(src)
            planes = np.ascontiguousarray(out["epf"][:, :src["height"], :src["width"]])
            got = backend.xyb(planes, np.array(p.opsin_matrix, np.float32), np.array(p.opsin_bias, np.float32),
                              np.array(p.cbrt_opsin_bias, np.float32), float(p.intensity_target))
            hold(name, "unfused inverse XYB", np.asarray(got), final)
    if final is None:
        return
    for what, switches in RESIDENT_SETS:
        out = R.decode(C.encoded(name), backend, cuts=False, **switches)
        hold(name, what, out["xyb"], final)
        if "device_output" in what:  # the image's planes came from the resident planes (JXLImage.resident), not from a host frame
            assert out["stats"][-1]["output"] == "device", (name, what, out["stats"][-1])
            hold(name, what + " image", np.stack([np.asarray(b) for b in out["image"].getBuffer()[:3]]), final)
