"""The PFM natives of integration/jni/jxlatte_amd_jni.c (stagePfmSamples, planesPfmSamples), called through ctypes over
tests/stubs/fake_jni.c as tests/test_jni_shim.py calls the others: they equal the C-ABI results, and their size checks -- the
output buffer must hold exactly the PFM's bytes -- arrive as the Java exception classes."""
import ctypes as C

import numpy as np
import pytest

from test_jni_shim import FakeJVM, _build


@pytest.mark.gpu
def test_pfm_sample_entries_over_jni_equal_the_c_abi(ctx, tmp_path):
    from jxlatte_amd import host
    vm = FakeJVM(_build(tmp_path))
    i32, i64, vp = C.c_int32, C.c_int64, C.c_void_p
    rng = np.random.default_rng(78)
    h, w = 19, 23
    src = [rng.normal(0, 2, (h, w)).astype(np.float32) for _ in range(3)]
    src[1].reshape(-1)[::5] = np.array([0xffa00001], np.uint32).view(np.float32)[0]
    mixed = [src[0], rng.integers(-9, 5000, (h, w)).astype(np.int32), src[2]]
    exp = host.pfmSamples(ctx, src)
    exp_mixed = host.pfmSamples(ctx, mixed, [8, 12, 8])
    exp_grey = host.pfmSamples(ctx, mixed[1:2], [12])
    handle = vm.fn("create", i64, i32)(vm.env, None, 0)
    assert handle and vm.pending() is None
    self_ = vm.lib.fj_self(handle)
    stage = vm.fn("stagePfmSamples", None, vp, vp, vp, vp, vp)
    resident = vm.fn("planesPfmSamples", None, vp, vp)
    upload = vm.fn("planesUpload", None, vp, vp, vp, i32, i32)
    orient = vm.fn("planesOrient", None, i32)
    floats = vm.ints([h, w, 3, 0, 0, 0, 0, 0, 0])
    try:
        out = np.zeros(exp.shape, exp.dtype)
        stage(vm.env, self_, vm.direct(src[0]), vm.direct(src[1]), vm.direct(src[2]), floats, vm.direct(out))
        assert vm.pending() is None, vm.pending()
        assert np.array_equal(out, exp)
        stage(vm.env, self_, vm.direct(mixed[0]), vm.direct(mixed[1]), vm.direct(mixed[2]), vm.ints([h, w, 3, 0, 1, 0, 8, 12, 8]), vm.direct(out))
        assert vm.pending() is None, vm.pending()
        assert np.array_equal(out, exp_mixed)
        grey = np.zeros(exp_grey.shape, exp_grey.dtype)
        stage(vm.env, self_, vm.direct(mixed[1]), None, None, vm.ints([h, w, 1, 1, 0, 0, 12, 0, 0]), vm.direct(grey))
        assert vm.pending() is None, vm.pending()
        assert np.array_equal(grey, exp_grey)
        # the resident entry: planes up, the same bytes; after an orientation that exchanges the sides the old geometry is refused
        upload(vm.env, self_, vm.direct(src[0]), vm.direct(src[1]), vm.direct(src[2]), h, w)
        assert vm.pending() is None, vm.pending()
        out2 = np.zeros(exp.shape, exp.dtype)
        resident(vm.env, self_, floats, vm.direct(out2))
        assert vm.pending() is None, vm.pending()
        assert np.array_equal(out2, exp)
        orient(vm.env, self_, 6)
        assert vm.pending() is None, vm.pending()
        resident(vm.env, self_, floats, vm.direct(out2))
        assert vm.take()[0] == "java/lang/IllegalArgumentException"
        # size checks: an output one byte short, one byte long, a short plane, a missing plane, a short parameter array, bad counts
        before = out.copy()
        for nbytes in (out.nbytes - 1, out.nbytes - 4):
            stage(vm.env, self_, vm.direct(src[0]), vm.direct(src[1]), vm.direct(src[2]), floats, vm.direct(out, nbytes))
            assert vm.take()[0] == "java/lang/IllegalArgumentException" and np.array_equal(out, before)
        longer = np.zeros(out.nbytes + 1, np.uint8)
        stage(vm.env, self_, vm.direct(src[0]), vm.direct(src[1]), vm.direct(src[2]), floats, vm.direct(longer))
        assert vm.take()[0] == "java/lang/IllegalArgumentException" and not longer.any()
        resident(vm.env, self_, vm.ints([w, h, 3, 0, 0, 0, 0, 0, 0]), vm.direct(longer))
        assert vm.take()[0] == "java/lang/IllegalArgumentException" and not longer.any()
        stage(vm.env, self_, vm.direct(src[0]), vm.direct(src[1], src[1].nbytes - 4), vm.direct(src[2]), floats, vm.direct(out))
        assert vm.take()[0] == "java/lang/IllegalArgumentException"
        stage(vm.env, self_, vm.direct(src[0]), None, vm.direct(src[2]), floats, vm.direct(out))
        assert vm.take()[0] == "java/lang/IllegalArgumentException"
        stage(vm.env, self_, vm.direct(src[0]), vm.direct(src[1]), vm.direct(src[2]), vm.ints([h, w, 3, 0, 0, 0, 0, 0]), vm.direct(out))
        assert vm.take()[0] == "java/lang/IllegalArgumentException"
        stage(vm.env, self_, vm.direct(src[0]), vm.direct(src[1]), vm.direct(src[2]), vm.ints([h, w, 2, 0, 0, 0, 0, 0, 0]), vm.direct(out))
        assert vm.take()[0] == "java/lang/IllegalArgumentException"
        # the library's own refusal comes through as the same class: an integer plane whose depth has no maximum
        stage(vm.env, self_, vm.direct(mixed[0]), vm.direct(mixed[1]), vm.direct(mixed[2]), vm.ints([h, w, 3, 0, 1, 0, 8, 32, 8]), vm.direct(out))
        assert vm.take()[0] == "java/lang/IllegalArgumentException" and np.array_equal(out, before)
        fresh = vm.fn("create", i64, i32)(vm.env, None, 0)
        resident(vm.env, vm.lib.fj_self(fresh), floats, vm.direct(out2))
        assert vm.take()[0] == "java/lang/IllegalStateException"
        vm.fn("destroy", None, i64)(vm.env, None, fresh)
    finally:
        vm.fn("destroy", None, i64)(vm.env, None, handle)
