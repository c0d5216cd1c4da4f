"""GPU: the cases of tests/jxl_writer_features_cases.py -- patches and splines inside a VarDCT frame, reference slots filled before and
after the colour transform, splines and noise inside a Modular frame -- through JXLDecoder on the device backend under nine switch
sets, from the default one to everything together. Every frame, every slot and the image are held to the float64 models of the SOURCE
under the K of jxl_writer_features_run, the same as the oracle backend on the CPU; no oracle and no second decode in those assertions.
Then the route each set promises (stats), the same bits from the same decode twice, and the spline and patch stage entries on the
cases' own planes."""
import numpy as np
import pytest

import jxl_writer_cases as WC
import jxl_writer_features_cases as FC
import jxl_writer_features_run as FR
import vardct_ref64 as M
from jxlatte_amd import host
from jxlatte_amd.decoder import DeviceBackend

pytestmark = pytest.mark.gpu
BOTH = dict(device_splines=True, device_patches=True)
SETS = (("default", {}), ("sparse_coeffs", dict(sparse_coeffs=True)), ("device_splines", dict(device_splines=True)),
        ("device_patches", dict(device_patches=True)), ("device_splines + device_patches", BOTH),
        ("device_splines + device_patches + device_output", dict(BOTH, device_output=True)),
        ("device_canvas + device_patches + device_patch_sets", dict(device_canvas=True, device_patches=True, device_patch_sets=True)),
        ("chains", WC.CHAINS),
        ("everything", dict(WC.CHAINS, sparse_coeffs=True, device_splines=True, device_output=True, device_image=True, device_palette=True)))


class Backend(DeviceBackend):
    """the device backend on the session's context"""

    def __init__(self, ctx):
        self.host, self.ctx = host, ctx
        self.palette_log = []


@pytest.fixture(scope="module")
def backend(ctx):
    return Backend(ctx)


def hold(name, what, out):
    c = FC.case(name)
    rows = FR.frame_ratios(name, out)
    assert {(i, cut) for i, cut, _, _, _ in rows} >= {(len(c["frames"]) - 1, "image")}
    for i, cut, r, k, row in rows:
        print("%s, %s, frame / slot %d %s: needs K = %.3f of %s (%s)" % (name, what, i, cut, r, k, row))
        assert k is not None and r <= k, (name, what, i, cut, r, k, row)
    return rows


def route(name, what, switches, out, traced):
    """what the switch set promises of the last frame's route"""
    c = FC.case(name)
    fr, st = c["frames"][-1], out["stats"][-1]
    print("%s, %s: %r" % (name, what, {k: st.get(k) for k in ("patches", "plane_moves", "output", "canvas", "frame")}))
    filled = any(f.get("save_as_reference") is not None and not f.get("is_last", f.get("type", 0) == 0) for f in c["frames"][:-1])
    # device_output's direct path: the frame IS the image -- the stream's only frame (a reference-only frame before it has made the
    # canvas, JXLCodestreamDecoder.java:640-643), of the image's size after upsampling
    h, w = fr["planes"][0].shape if FC.is_modular(fr) else (fr["height"], fr["width"])
    k = fr.get("upsampling", 1)
    direct = bool(switches.get("device_output")) and len(c["frames"]) == 1 and (h * k, w * k) == (c["image"]["height"], c["image"]["width"])
    if fr.get("patches"):
        path = st["patches"]["path"]
        if switches.get("device_patch_sets") and switches.get("device_canvas") and not direct:
            assert path == "plane sets" and st["canvas"] == "device", (name, what, st)
        elif switches.get("device_patches"):
            assert path == ("resident planes" if filled else "none"), (name, what, st)
        else:
            assert path == "blend calls", (name, what, st)
    if direct:
        assert st["output"] == "device", (name, what, st)
    elif switches.get("device_canvas"):
        assert st["canvas"] == "device", (name, what, st)
    resident = (direct or switches.get("device_canvas")) and not FC.is_modular(fr)
    if resident and (switches.get("device_splines") or not fr.get("splines")) and (switches.get("device_patches") or not fr.get("patches")):
        # every stage of the tail ran where the planes are: the only copy is this test's own trace listener's
        assert [m for m in st.get("plane_moves", []) if m != "trace"] == [], (name, what, st)
    if not FC.is_modular(fr) and switches.get("device_frames") and not direct:  # frame_set_rule's first answer, in a real decode
        assert st["frame"] == "host: not a Modular frame", (name, what, st)
    if FC.is_modular(fr) and switches.get("device_frames") and not traced and not direct:
        if c["image"].get("xyb", False):  # frame_set_rule: a frame of an XYB image stays with the host route
            assert st["frame"] == "host: an XYB image", (name, what, st)
        else:  # the resident tail: splines between jxl_canvas_to_planes and jxl_canvas_take_planes
            assert st["frame"] == "device set (modular)", (name, what, st)
            if switches.get("device_splines") or not fr.get("splines"):
                assert [m for m in st.get("plane_moves", []) if m != "trace"] == [], (name, what, st)


@pytest.mark.parametrize("name", FC.NAMES)
def test_device_decode_is_the_model(name, backend):
    data = FC.encoded(name)
    modular = FC.is_modular(FC.case(name)["frames"][-1])
    for what, switches in SETS:
        out = FR.decode(data, backend, **switches)
        rows = hold(name, what, out)
        assert (len(FC.case(name)["frames"]) - 1, "xyb") in {(i, cut) for i, cut, _, _, _ in rows}
        route(name, what, switches, out, True)
        if modular and switches.get("device_frames"):  # a listener keeps a frame off the device sets: once more without one
            out = FR.decode(data, backend, trace=False, **switches)
            hold(name, what + ", no listener", out)
            route(name, what + ", no listener", switches, out, False)


@pytest.mark.parametrize("name", FC.NAMES)
def test_the_same_decode_twice_gives_the_same_bits(name, backend):
    data = FC.encoded(name)
    for what, switches in (SETS[0], SETS[4], SETS[8]):
        a = FR.decode(data, backend, trace=False, **switches)["image"].getBuffer()
        b = FR.decode(data, backend, trace=False, **switches)["image"].getBuffer()
        assert all(np.array_equal(np.asarray(p).view(np.uint32), np.asarray(q).view(np.uint32)) for p, q in zip(a, b)), (name, what)


@pytest.mark.parametrize("name", FR.STAGE_CASES)
def test_the_spline_entries_on_a_case_s_own_planes(name, ctx):
    """host.renderSplines (jxl_stage_splines) and ResidentPlanes.splines (jxl_planes_splines) on the model's float32 planes in front
    of the spline stage, against the float64 model under the stage's K, measured on the host render"""
    planes, splines, bx, bb, (x, a) = FR.spline_stage(name)
    staged = host.renderSplines(ctx, planes, splines, bx, bb)
    rp = host.ResidentPlanes.upload(ctx, planes)
    rp.splines(splines, bx, bb)
    resident = np.stack(rp.download())
    for what, got in (("jxl_stage_splines", staged), ("jxl_planes_splines", resident)):
        r = M.error_ratio(got, x, a)
        print("%s %s: needs K = %.2f of %d" % (name, what, r, FR.K_SPLINE_STAGE))
        assert got.dtype == np.float32 and r <= FR.K_SPLINE_STAGE, (name, what, r)
    assert np.array_equal(staged.view(np.uint32), resident.view(np.uint32)), name


@pytest.mark.parametrize("name", FR.PATCH_STAGE_CASES)
def test_the_patch_entries_on_a_case_s_own_planes(name, ctx):
    """host.computePatches (jxl_stage_patches) and ResidentPlanes.patches (jxl_planes_patches) on the model's float32 planes in front
    of the patch stage and the model's slots, against the float64 patch stage under the K derived from the SOURCE: sums from a
    Modular and from a VarDCT slot, an upsampled frame, and BLEND and MULADD through an alpha channel"""
    planes, slots, pos, blend, (x, a), k = FR.patch_stage(name)
    n_extra = planes.shape[0] - 3
    is_alpha, assoc = [True] * n_extra, [False] * n_extra
    staged = np.stack(host.computePatches(ctx, [planes[c].copy() for c in range(3 + n_extra)], slots, pos, blend, 3, is_alpha, assoc))
    rp = host.ResidentPlanes.upload(ctx, planes[:3])
    extras = [planes[c].copy() for c in range(3, 3 + n_extra)]
    rp.patches(extras, slots, pos, blend, is_alpha, assoc)
    resident = np.stack(list(rp.download()) + extras)
    for what, got in (("jxl_stage_patches", staged), ("jxl_planes_patches", resident)):
        r = M.error_ratio(got, x, a)
        print("%s %s: needs K = %.2f of %d" % (name, what, r, k))
        assert got.dtype == np.float32 and r <= k, (name, what, r)
    assert all((staged[c] != planes[c]).any() for c in range(3 + n_extra))
