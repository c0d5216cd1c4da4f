"""The natives of integration/jni/jxlatte_amd_jni.c that device_frames adds (canvasFromModularUp, canvasTakePlanes), called through
ctypes over tests/stubs/fake_jni.c as tests/test_jni_shim_pfm.py calls the others: they equal the C-ABI results, and their refusals
arrive as the Java exception classes."""
import ctypes as C

import numpy as np
import pytest

from test_jni_shim import FakeJVM, _build


@pytest.mark.gpu
def test_frame_set_entries_over_jni_equal_the_c_abi(ctx, tmp_path):
    from conftest import assert_bits_equal
    from jxlatte_amd import host
    from jxlatte_amd.upweights import DEFAULT_UP
    vm = FakeJVM(_build(tmp_path))
    i32, i64, vp, f32 = C.c_int32, C.c_int64, C.c_void_p, C.c_float
    vm.lib.fj_objects.restype, vm.lib.fj_objects.argtypes = vp, [i64]
    vm.lib.fj_set_object.restype, vm.lib.fj_set_object.argtypes = None, [vp, i64, vp]

    def floats(a):
        a = np.ascontiguousarray(a, np.float32)
        vm.keep.append(a)
        return vm.lib.fj_floats(a.ctypes.data, a.size)
    rng = np.random.default_rng(41)
    h, w, k = 9, 13, 2
    chans = [rng.integers(-5, 4100, (12, 17)).astype(np.int32) for _ in range(4)]
    planes = [(0, -1, np.float32, 1.0 / 255), (1, -1, np.float32, 1.0 / 4095), (2, 3, np.float32, 0.5), (3, -1, np.float32, 1.0)]
    wts = host.getUpWeights(k, DEFAULT_UP[k])
    lut = np.linspace(0.05, 0.6, 8).astype(np.float32)
    # the C ABI on the session's context
    host.ModularStream(ctx, chans, []).run()
    cv = host.DeviceCanvas.fromModularUp(ctx, h, w, planes, k, wts)
    exp = [cv.download(c) for c in range(4)]
    rp = cv.toPlanes()
    rp.noise(256, 7, lut, 0.0, 1.0)
    cv.takePlanes()
    exp_taken = [cv.download(c) for c in range(4)]
    cv.release()
    assert not np.array_equal(exp[0], exp_taken[0]) and np.array_equal(exp[3], exp_taken[3])
    # the same calls over JNI, on a context of the shim's own
    handle = vm.fn("create", i64, i32)(vm.env, None, 0)
    assert handle and vm.pending() is None
    self_ = vm.lib.fj_self(handle)
    from_up = vm.fn("canvasFromModularUp", i32, vp, vp, i32, vp)
    take = vm.fn("canvasTakePlanes", None, i32)
    download = vm.fn("canvasDownload", i32, i32, i32, vp)
    desc = vm.ints([h, w, 4] + [v for ch, add, _, _ in planes for v in (ch, add, 0)])
    scales = floats([p[3] for p in planes])

    def planes_of(id_):
        out = []
        for c in range(4):
            a = np.zeros((h * k, w * k), np.float32)
            assert download(vm.env, self_, id_, c, vm.direct(a)) == 0 and vm.pending() is None, vm.pending()
            out.append(a)
        return out
    try:
        arr = vm.lib.fj_objects(len(chans))
        for i, a in enumerate(chans):
            vm.lib.fj_set_object(arr, i, vm.direct(a))
        vm.fn("modularBegin", None, vp, vp, vp, vp, i32, i32)(vm.env, self_, arr, vm.ints([17] * 4), vm.ints([12] * 4), vm.ints([]), -1, 0)
        assert vm.pending() is None, vm.pending()
        vm.fn("modularRun", None)(vm.env, self_)
        assert vm.pending() is None, vm.pending()
        id_ = from_up(vm.env, self_, desc, scales, k, floats(wts))
        assert vm.pending() is None and id_ >= 0, vm.pending()
        for c, a in enumerate(planes_of(id_)):
            assert_bits_equal(a, exp[c], "canvasFromModularUp, plane %d" % c)
        vm.fn("canvasToPlanes", None, i32)(vm.env, self_, id_)
        assert vm.pending() is None, vm.pending()
        vm.fn("planesNoise", None, i32, i64, vp, f32, f32)(vm.env, self_, 256, 7, floats(lut), 0.0, 1.0)
        assert vm.pending() is None, vm.pending()
        take(vm.env, self_, id_)
        assert vm.pending() is None, vm.pending()
        for c, a in enumerate(planes_of(id_)):
            assert_bits_equal(a, exp_taken[c], "canvasTakePlanes, plane %d" % c)
        # refusals: the library's arrive as the Java classes, the shim's own size checks too; no set is made
        assert from_up(vm.env, self_, desc, scales, 3, floats(wts)) == -1
        assert vm.take()[0] == "java/lang/IllegalArgumentException"
        assert from_up(vm.env, self_, desc, scales, k, floats(wts.reshape(-1)[:-1])) == -1
        assert vm.take()[0] == "java/lang/IllegalArgumentException"
        assert from_up(vm.env, self_, desc, scales, k, None) == -1
        assert vm.take()[0] == "java/lang/IllegalArgumentException"
        int_plane = vm.ints([h, w, 4] + [v for ch, add, _, _ in planes for v in (ch, add, 1)])
        assert from_up(vm.env, self_, int_plane, scales, k, floats(wts)) == -1
        assert vm.take()[0] == "java/lang/IllegalArgumentException"
        assert from_up(vm.env, self_, vm.ints([h, w, 17]), scales, k, floats(wts)) == -1
        assert vm.take()[0] == "java/lang/UnsupportedOperationException"
        assert from_up(vm.env, self_, desc, scales, k, floats(wts)) == id_ + 1  # (the next id: the refusals made none)
        assert vm.pending() is None, vm.pending()
        take(vm.env, self_, 9999)
        assert vm.take()[0] == "java/lang/IllegalArgumentException"
        fresh = vm.fn("create", i64, i32)(vm.env, None, 0)
        fself = vm.lib.fj_self(fresh)
        fid = vm.fn("canvasCreate", i32, i32, i32, vp)(vm.env, fself, 4, 4, vm.ints([0, 0, 0]))
        assert vm.pending() is None and fid >= 0, vm.pending()
        take(vm.env, fself, fid)
        assert vm.take()[0] == "java/lang/IllegalStateException"
        vm.fn("destroy", None, i64)(vm.env, None, fresh)
    finally:
        vm.fn("destroy", None, i64)(vm.env, None, handle)
