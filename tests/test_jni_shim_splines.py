"""The spline natives of integration/jni/jxlatte_amd_jni.c (splineArcs, stageSplines, planesSplines), called through ctypes over
tests/stubs/fake_jni.c as tests/test_jni_shim.py calls the others: they equal the C-ABI results, and their argument checks arrive
as the Java exception classes."""
import ctypes as C

import numpy as np
import pytest

import spline_ref as R
from test_jni_shim import FakeJVM, _build


def _flat(splines):
    n_control = [len(s["control"]) for s in splines]
    control = [v for s in splines for p in s["control"] for v in p]
    coeff = [v for s in splines for row in s["coeff"] for v in row]
    return n_control, control, coeff


@pytest.mark.gpu
def test_spline_entries_over_jni_equal_the_c_abi(ctx, tmp_path):
    from jxlatte_amd import abi, host
    vm = FakeJVM(_build(tmp_path))
    i32, i64, vp, f32 = C.c_int32, C.c_int64, C.c_void_p, C.c_float
    h, w = 70, 100
    splines, planes = R.random_splines(61, 4, h, w, sigma=(3, 12), margin=10), R.random_planes(62, h, w)
    nc, cp, cf = _flat(splines)
    exp = host.renderSplines(ctx, planes, splines, -0.125, 0.875)
    handle = vm.fn("create", i64, i32)(vm.env, None, 0)
    assert handle and vm.pending() is None
    self_ = vm.lib.fj_self(handle)
    arcs_fn = vm.fn("splineArcs", vp, i32, i32, i32, vp, vp, vp, f32, f32)
    stage = vm.fn("stageSplines", None, vp, vp, vp, i32, i32, i32, vp, vp, vp, f32, f32)
    resident = vm.fn("planesSplines", None, i32, vp, vp, vp, f32, f32)
    upload = vm.fn("planesUpload", None, vp, vp, vp, i32, i32)
    download = vm.fn("planesDownload", None, vp, vp, vp)
    try:
        # the arc table, word for word
        arr = arcs_fn(vm.env, None, h, w, 0, vm.ints(nc), vm.ints(cp), vm.ints(cf), -0.125, 0.875)
        assert vm.pending() is None and arr, vm.pending()
        table = host.spline_arcs(splines, -0.125, 0.875, h, w)
        assert vm.lib.fj_length(arr) == 12 * len(table)
        words = np.ctypeslib.as_array(C.cast(vm.lib.fj_data(arr), C.POINTER(C.c_int32)), shape=(12 * len(table),))
        assert np.array_equal(words, table.view(np.int32).reshape(-1))
        # the stage on host planes
        out = [planes[c].copy() for c in range(3)]
        stage(vm.env, self_, vm.direct(out[0]), vm.direct(out[1]), vm.direct(out[2]), h, w, 0, vm.ints(nc), vm.ints(cp), vm.ints(cf), -0.125, 0.875)
        assert vm.pending() is None, vm.pending()
        assert np.array_equal(np.stack(out).view(np.uint32), exp.view(np.uint32))
        # ... and on the resident planes
        src = [planes[c].copy() for c in range(3)]
        upload(vm.env, self_, vm.direct(src[0]), vm.direct(src[1]), vm.direct(src[2]), h, w)
        assert vm.pending() is None, vm.pending()
        resident(vm.env, self_, 0, vm.ints(nc), vm.ints(cp), vm.ints(cf), -0.125, 0.875)
        assert vm.pending() is None, vm.pending()
        got = [np.zeros((h, w), np.float32) for _ in range(3)]
        download(vm.env, self_, vm.direct(got[0]), vm.direct(got[1]), vm.direct(got[2]))
        assert vm.pending() is None, vm.pending()
        assert np.array_equal(np.stack(got).view(np.uint32), exp.view(np.uint32))
        # argument checks: a plane buffer too small, a control array shorter than the counts say, a short coefficient array, a
        # spline without points, null arrays, no resident planes
        stage(vm.env, self_, vm.direct(out[0], out[0].nbytes - 4), vm.direct(out[1]), vm.direct(out[2]), h, w, 0, vm.ints(nc), vm.ints(cp), vm.ints(cf), 0.0, 1.0)
        assert vm.take()[0] == "java/lang/IllegalArgumentException"
        stage(vm.env, self_, vm.direct(out[0]), vm.direct(out[1]), vm.direct(out[2]), h, w, 0, vm.ints(nc), vm.ints(cp[:-2]), vm.ints(cf), 0.0, 1.0)
        assert vm.take()[0] == "java/lang/IllegalArgumentException"
        stage(vm.env, self_, vm.direct(out[0]), vm.direct(out[1]), vm.direct(out[2]), h, w, 0, vm.ints(nc), vm.ints(cp), vm.ints(cf[:-1]), 0.0, 1.0)
        assert vm.take()[0] == "java/lang/IllegalArgumentException"
        stage(vm.env, self_, vm.direct(out[0]), vm.direct(out[1]), vm.direct(out[2]), h, w, 0, vm.ints([0] + nc[1:]), vm.ints(cp), vm.ints(cf), 0.0, 1.0)
        assert vm.take()[0] == "java/lang/IllegalArgumentException"
        arcs_fn(vm.env, None, h, w, 0, None, vm.ints(cp), vm.ints(cf), 0.0, 1.0)
        assert vm.take()[0] == "java/lang/IllegalArgumentException"
        arcs_fn(vm.env, None, 0, w, 0, vm.ints(nc), vm.ints(cp), vm.ints(cf), 0.0, 1.0)
        assert vm.take()[0] == "java/lang/IllegalArgumentException"
        fresh = vm.fn("create", i64, i32)(vm.env, None, 0)
        resident(vm.env, vm.lib.fj_self(fresh), 0, vm.ints(nc), vm.ints(cp), vm.ints(cf), 0.0, 1.0)
        assert vm.take()[0] == "java/lang/IllegalStateException"
        vm.fn("destroy", None, i64)(vm.env, None, fresh)
    finally:
        vm.fn("destroy", None, i64)(vm.env, None, handle)
