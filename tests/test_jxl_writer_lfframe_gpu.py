"""GPU: the cases of tests/jxl_writer_lfframe_cases.py -- LF frames, frames that copy their LF out of one, permuted TOCs -- through
JXLDecoder on the device backend, under the default switches, sparse_coeffs, and the sets that keep a frame's planes resident
(device_output, device_canvas, and both with the sparse feed). Every frame is held to the float64 models of the SOURCE under the K of
jxl_writer_lfframe_run.bound, the same as the oracle backend on the CPU; no oracle and no second decode in those assertions.

A consumer's LF planes are host arrays cut out of lfBuffer that reach the device through the LF-group entry as three bare pointers: the
sizes that entry is given here are 5 x 9, 9 x 17, 2 x 256 and 2 x 1 cells. An LF frame's planes come down under every switch set:
lfBuffer holds host float32 (or int32) planes of the frame's padded size."""
import numpy as np
import pytest

import jxl_writer_lfframe_cases as L
import jxl_writer_lfframe_run as LR
import jxl_writer_vardct as V
from jxlatte_amd import host
from jxlatte_amd.decoder import DeviceBackend, JXLDecoder, UnsupportedOperationException

pytestmark = pytest.mark.gpu
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


def hold(name, what, out, cuts):
    rows = LR.frame_ratios(name, out, cuts=cuts)
    frames = L.case(name)["frames"]
    assert {(i, cut) for i, cut, _, _, _ in rows} >= {(i, "stored") for i, f in enumerate(frames) if f.get("lf_level", 0)} | \
        {(len(frames) - 1, "image"), (len(frames) - 1, "xyb")}
    for i, cut, r, k, row in rows:
        print("%s, %s, frame %d %s: needs K = %.3f of %s (%s)" % (name, what, i, cut, r, k, row))
        assert r <= (k or 0), (name, what, i, cut, r, k)
    for slot, planes in enumerate(out["lfBuffer"]):  # host planes of the LF frame's padded size
        src = [f for f in frames if f.get("lf_level", 0) == slot + 1]
        assert (planes is None) == (not src), (name, what, slot)
        if src:
            want = src[-1]["planes"][0].shape if L.is_modular(src[-1]) else V.padded_size(src[-1])
            assert all(isinstance(p, np.ndarray) and p.shape == want for p in planes), (name, what, slot)
    for fr, st in zip(frames, out["stats"]):  # an LF frame's planes come down whole; no stage of a tail ever holds them
        if fr.get("lf_level", 0):
            assert st["output"] == "host" and "plane_moves" not in st, (name, what, st)


@pytest.mark.parametrize("name", L.NAMES)
def test_device_decode_is_the_model(name, backend):
    data = L.encoded(name)
    n_vardct = sum(1 for f in L.case(name)["frames"] if not L.is_modular(f))
    for what, switches in CUT_SETS:
        out = LR.decode(data, backend, **switches)
        assert out["vardct_calls"] == n_vardct
        hold(name, what, out, True)
    for what, switches in RESIDENT_SETS:
        out = LR.decode(data, backend, cuts=False, **switches)
        hold(name, what, out, False)
        st = out["stats"][-1]
        print("%s, %s: %r" % (name, what, {k: st.get(k) for k in ("plane_moves", "output", "canvas")}))
        if "device_output" in what:  # the last frame is the image: its own resident planes are handed out
            assert st["output"] == "device", (name, what, st)
        else:
            assert st["canvas"] == "device", (name, what, st)
        # the colours never came down for a stage: the only copy is this test's own trace listener's
        assert [m for m in st.get("plane_moves", ["trace"]) if m != "trace"] == [], (name, what, st)


def test_a_preview_and_a_region_of_a_stream_with_an_lf_frame_are_refused(backend):
    data = L.encoded("lf1_vardct")
    with pytest.raises(UnsupportedOperationException) as e:
        JXLDecoder(data, backend=backend, downsample=8).decode()
    assert str(e.value) == "downsample=8: not a regular frame of LF level 0 with LF coefficients of its own"
    with pytest.raises(UnsupportedOperationException) as e:
        JXLDecoder(data, backend=backend, region=(0, 0, 16, 16)).decode()
    assert str(e.value) == "region: not a regular frame of LF level 0 with LF coefficients of its own"


@pytest.mark.parametrize("box", ((0, 0, 40, 40), (250, 250, 14, 14), (100, 200, 100, 64)))
def test_a_region_of_a_permuted_frame_is_the_crop_of_the_full_decode(box, backend):
    x0, y0, w, h = box
    data = L.encoded("toc_perm_groups")
    full = JXLDecoder(data, backend=backend).decode().getBuffer()
    dec = JXLDecoder(data, backend=backend, region=box)
    got = dec.decode().getBuffer()
    for c in range(3):
        assert got[c].dtype == np.float32 and np.array_equal(got[c].view(np.uint32), full[c][y0:y0 + h, x0:x0 + w].view(np.uint32)), (box, c)
    assert dec.stats[-1]["region"]["path"] == "groups"


def test_device_frames_leaves_a_modular_lf_frame_to_the_host(backend):
    """frame_set_rule: an LF frame never reaches the canvas as a plane set; the stream decodes as without the switch"""
    data = L.encoded("lf1_modular_xyb")
    out = LR.decode(data, backend, cuts=False, trace=False, device_frames=True, device_canvas=True)
    assert out["stats"][0]["frame"] == "host: not a regular or skip-progressive frame of LF level 0", out["stats"][0]
    assert out["stats"][1]["frame"] == "host: not a Modular frame", out["stats"][1]
    rows = LR.frame_ratios("lf1_modular_xyb", out, cuts=False)
    assert {cut for _, cut, _, _, _ in rows} == {"stored", "image"}
    for i, cut, r, k, row in rows:
        print("lf1_modular_xyb, device_frames, frame %d %s: needs K = %.3f of %s" % (i, cut, r, k))
        assert r <= k, (i, cut, r, k)
