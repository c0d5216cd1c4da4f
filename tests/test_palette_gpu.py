"""jxl_stage_palette on the device against the Python model of tests/palette_ref.py (ModularStream.java:327-378), exactly, on
every case of tests/palette_cases.py: every index class, every predictor, palette entries that make the sums wrap, the shapes at
which the kernels take another path (the last group of 4, more than one workgroup, a t-front longer than the chain kernel's
workgroup, a palette that fills the LDS budget and one that does not fit). The launch count comes from jxl_debug_last_palette, a
hook outside the C ABI."""
import ctypes as C

import numpy as np
import pytest

import palette_cases
from jxlatte_amd import _lib, abi, host

pytestmark = pytest.mark.gpu
NAMES = sorted(palette_cases.CASES)


def _run(ctx, name):
    c = palette_cases.CASES[name]
    return host.inversePalette(ctx, c["index"], c["palette"], c["num_c"], c["nb_colors"], c["nb_deltas"], c["d_pred"], c["bit_depth"],
                               pred=c["pred"])


@pytest.mark.parametrize("name", NAMES)
def test_stage_equals_the_model_and_launches_what_it_must(ctx, name):
    c = palette_cases.CASES[name]
    index = c["index"].copy()
    got = _run(ctx, name)
    want = palette_cases.expected(name)
    assert got.shape == want.shape and got.dtype == np.int32
    bad = np.argwhere(got != want)
    assert bad.size == 0, "%s: %d samples differ, the first at (c, y, x) = %s: %d, expected %d" % (
        name, len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])
    launches, deltas = host.lastPalette(ctx)
    assert launches == palette_cases.launches(name)
    assert deltas == int((c["index"] < c["nb_deltas"]).sum())
    assert np.array_equal(index, c["index"])  # the input is not written


@pytest.mark.parametrize("name", ["pred13_33x70", "pred06_21x37", "lds_over_4x2049", "shape_1x1_0_pred04"])
def test_first_output_plane_may_be_the_index_plane(ctx, name):
    c = palette_cases.CASES[name]
    want = palette_cases.expected(name)
    idx = np.ascontiguousarray(c["index"]).copy()
    rest = np.empty((c["num_c"] - 1,) + idx.shape, np.int32)
    planes = [idx] + list(rest)
    d, keep = abi.make_palette_desc(c["palette"], c["pred"], c["num_c"], c["nb_colors"], c["nb_deltas"], c["d_pred"], c["bit_depth"])
    pp = (C.POINTER(C.c_int32) * len(planes))(*[abi.iptr(a) for a in planes])
    ctx.call("jxl_stage_palette", C.byref(d), abi.iptr(idx), c["h"], c["w"], pp)
    assert all(np.array_equal(planes[k], want[k]) for k in range(c["num_c"]))


def _refusals():
    """(name, changes to a good call): the refusals of section "what jxl_stage_palette refuses" of include/jxlatte_amd.h"""
    return [("null_desc", dict(desc=None)), ("null_index", dict(index=None)), ("null_out", dict(out=None)),
            ("null_out_plane", dict(hole=True)), ("null_palette", dict(palette=None)),
            ("height_0", dict(h=0)), ("width_0", dict(w=0)), ("height_negative", dict(h=-21)), ("width_negative", dict(w=-(1 << 31))),
            ("too_many_samples", dict(h=65536, w=32768)),
            ("num_c_0", dict(num_c=0)), ("num_c_negative", dict(num_c=-3)), ("nb_colors_negative", dict(nb_colors=-1)),
            ("nb_deltas_negative", dict(nb_deltas=-1)), ("pal_w_below_nb_colors", dict(pal_w=-1)), ("pal_h_below_num_c", dict(pal_h=-1)),
            ("d_pred_negative", dict(d_pred=-1)), ("d_pred_14", dict(d_pred=14)), ("d_pred_6_without_pred", dict(d_pred=6, pred=None)),
            ("bit_depth_0", dict(bit_depth=0)), ("bit_depth_33", dict(bit_depth=33))]


@pytest.mark.parametrize("what,change", _refusals(), ids=[r[0] for r in _refusals()])
def test_refusals_leave_the_outputs_untouched_and_the_context_usable(ctx, what, change):
    name = "pred05_33x70"  # nb_deltas > 0, three channels, a palette channel wider and taller than it has to be
    c = palette_cases.CASES[name]
    idx = np.ascontiguousarray(c["index"])
    out = np.full((c["num_c"],) + idx.shape, 0x5a5a5a5a, np.int32)
    pred = np.zeros(idx.shape, np.int32)
    d, keep = abi.make_palette_desc(c["palette"], pred, c["num_c"], c["nb_colors"], c["nb_deltas"], c["d_pred"], c["bit_depth"])
    h, w = c["h"], c["w"]
    for k, v in change.items():
        if k in ("num_c", "nb_colors", "nb_deltas", "d_pred", "bit_depth"):
            setattr(d, k, v)
        elif k == "pal_w":
            d.pal_w = c["nb_colors"] + v
        elif k == "pal_h":
            d.pal_h = c["num_c"] + v
        elif k in ("palette", "pred"):
            setattr(d, k, None)
    h, w = change.get("h", h), change.get("w", w)
    planes = [abi.iptr(a) for a in out]
    if change.get("hole"):
        planes[1] = None
    pp = None if "out" in change else (C.POINTER(C.c_int32) * len(planes))(*planes)
    st = ctx.lib.jxl_stage_palette(ctx.h, None if "desc" in change else C.byref(d), None if "index" in change else abi.iptr(idx), h, w, pp)
    assert st == abi.JXL_ERR_INVALID_ARGUMENT, (what, st)
    assert (out == 0x5a5a5a5a).all()
    # the context goes on: a good call behind the refusal gives the model's planes
    assert np.array_equal(_run(ctx, "pred04_21x37"), palette_cases.expected("pred04_21x37"))
