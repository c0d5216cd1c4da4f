"""The palette native of integration/jni/jxlatte_amd_jni.c (stagePalette), called through ctypes over tests/stubs/fake_jni.c as
tests/test_jni_shim.py calls the others: it equals the C-ABI result, and its size checks and the library's refusals arrive as
IllegalArgumentException with the outputs untouched."""
import ctypes as C

import numpy as np
import pytest

import palette_cases
from test_jni_shim import FakeJVM, _build


@pytest.mark.gpu
def test_palette_entry_over_jni_equals_the_c_abi(ctx, tmp_path):
    from jxlatte_amd import host
    vm = FakeJVM(_build(tmp_path))
    vm.lib.fj_objects.restype, vm.lib.fj_objects.argtypes = C.c_void_p, [C.c_int64]
    vm.lib.fj_set_object.restype, vm.lib.fj_set_object.argtypes = None, [C.c_void_p, C.c_int64, C.c_void_p]
    i32, i64, vp = C.c_int32, C.c_int64, C.c_void_p
    name = "pred04_21x37"  # three channels, delta pixels that chain, a palette channel wider than nb_colors
    c = palette_cases.CASES[name]
    assert (c["h"], c["w"]) == (21, 37) and c["num_c"] > 1
    h, w, nc = c["h"], c["w"], c["num_c"]
    idx, pal = np.ascontiguousarray(c["index"]), np.ascontiguousarray(c["palette"])
    params = [nc, c["nb_colors"], c["nb_deltas"], c["d_pred"], c["bit_depth"]]
    exp = host.inversePalette(ctx, idx, pal, *params, pred=c["pred"])
    assert np.array_equal(exp, palette_cases.expected(name))
    handle = vm.fn("create", i64, i32)(vm.env, None, 0)
    assert handle and vm.pending() is None
    self_ = vm.lib.fj_self(handle)
    stage = vm.fn("stagePalette", None, vp, i32, i32, vp, i32, i32, vp, vp, vp)

    def planes_of(arrays, sizes=None):
        arr = vm.lib.fj_objects(len(arrays))
        for k, a in enumerate(arrays):
            vm.lib.fj_set_object(arr, k, vm.direct(a, None if sizes is None else sizes[k]))
        return arr
    try:
        out = [np.full((h, w), -77, np.int32) for _ in range(nc)]
        stage(vm.env, self_, vm.direct(idx), h, w, vm.direct(pal), pal.shape[0], pal.shape[1], None, vm.ints(params), planes_of(out))
        assert vm.pending() is None, vm.pending()
        assert all(np.array_equal(out[k], exp[k]) for k in range(nc))
        # in place: out[0] is the index buffer
        inplace = [idx.copy()] + [np.zeros((h, w), np.int32) for _ in range(nc - 1)]
        stage(vm.env, self_, vm.direct(inplace[0]), h, w, vm.direct(pal), pal.shape[0], pal.shape[1], None, vm.ints(params), planes_of(inplace))
        assert vm.pending() is None, vm.pending()
        assert all(np.array_equal(inplace[k], exp[k]) for k in range(nc))
        # size checks: nothing reaches the library, the outputs stay
        fresh = [np.full((h, w), -77, np.int32) for _ in range(nc)]
        good = dict(index=vm.direct(idx), h=h, w=w, pal=vm.direct(pal), ph=pal.shape[0], pw=pal.shape[1], pred=None, params=vm.ints(params),
                    out=planes_of(fresh))

        def refused(**change):
            a = dict(good, **change)
            stage(vm.env, self_, a["index"], a["h"], a["w"], a["pal"], a["ph"], a["pw"], a["pred"], a["params"], a["out"])
            got = vm.take()
            assert got is not None and got[0] == "java/lang/IllegalArgumentException", (change, got)
            assert all((f == -77).all() for f in fresh), change
        refused(index=vm.direct(idx, idx.nbytes - 4))                         # a short index plane
        refused(index=None)                                                    # a null plane
        refused(pal=vm.direct(pal, pal.nbytes - 4))                           # a short palette
        refused(pal=None)
        refused(pred=vm.direct(np.zeros(h * w - 1, np.int32)))                # a short predictor plane
        refused(params=vm.ints(params[:4]))                                    # a short parameter array
        refused(params=None)
        refused(out=planes_of(fresh[:nc - 1]))                                 # fewer planes than numC
        refused(out=planes_of(fresh, [f.nbytes for f in fresh[:-1]] + [fresh[-1].nbytes - 1]))  # a short output plane
        short = vm.lib.fj_objects(nc)
        vm.lib.fj_set_object(short, 0, vm.direct(fresh[0]))
        refused(out=short)                                                     # a null output plane
        refused(out=None)
        refused(h=0)
        refused(w=-1)
        # the library's own refusals come through as the same class
        refused(params=vm.ints([nc, c["nb_colors"], c["nb_deltas"], 14, c["bit_depth"]]))
        refused(params=vm.ints([nc, c["nb_colors"], c["nb_deltas"], c["d_pred"], 33]))
        refused(params=vm.ints([nc, pal.shape[1] + 1, c["nb_deltas"], c["d_pred"], c["bit_depth"]]))
        refused(params=vm.ints([pal.shape[0] + 1, c["nb_colors"], c["nb_deltas"], c["d_pred"], c["bit_depth"]]),
                out=planes_of(fresh + [fresh[0]] * (pal.shape[0] + 1 - nc)))
        refused(params=vm.ints([nc, c["nb_colors"], 3, 6, c["bit_depth"]]))   # predictor 6 without its plane
        # a good call behind the refusals
        stage(vm.env, self_, good["index"], h, w, good["pal"], good["ph"], good["pw"], None, good["params"], good["out"])
        assert vm.pending() is None, vm.pending()
        assert all(np.array_equal(fresh[k], exp[k]) for k in range(nc))
    finally:
        vm.fn("destroy", None, i64)(vm.env, None, handle)
