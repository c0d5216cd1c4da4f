"""The plane-set natives of integration/jni/jxlatte_amd_jni.c (canvasCreate ... canvasBlendCheck), called through ctypes over
tests/stubs/fake_jni.c as tests/test_jni_shim.py calls the others: create, upload, blend, download equals the C-ABI, and the
capacity checks -- a transfer's buffer must hold a plane of the set -- arrive as the Java exception classes."""
import ctypes as C

import numpy as np
import pytest

from test_jni_shim import FakeJVM, _build


def _ints_of(vm, arr):
    n = vm.lib.fj_length(arr)
    return np.ctypeslib.as_array(C.cast(vm.lib.fj_data(arr), C.POINTER(C.c_int32)), (n,)).copy()


@pytest.mark.gpu
def test_canvas_entries_over_jni_equal_the_c_abi(ctx, tmp_path):
    from jxlatte_amd import abi, host
    vm = FakeJVM(_build(tmp_path))
    i32, i64, vp = C.c_int32, C.c_int64, C.c_void_p
    rng = np.random.default_rng(21)
    h, w, fh, fw = 19, 23, 10, 13
    canvas = [rng.normal(0.5, 1, (h, w)).astype(np.float32) for _ in range(3)] + [rng.random((h, w)).astype(np.float32)]
    frame = [rng.normal(0.5, 1, (fh, fw)).astype(np.float32) for _ in range(3)] + [rng.random((fh, fw)).astype(np.float32)]
    ints = rng.integers(0, 4095, (h, w)).astype(np.int32)
    he, ia = abi.BLEND_FLAG_HAS_EXTRA, abi.BLEND_FLAG_IS_ALPHA
    rect = [fh, fw, 4, 5, 0, 0, 4, 5]
    chans = [(c, abi.BLEND_BLEND, he | (ia if c == 3 else 0), 3, 3) for c in range(4)]
    # the C-ABI
    cv, fs = host.DeviceCanvas.fromArrays(ctx, canvas), host.DeviceCanvas.fromArrays(ctx, frame)
    host.canvas_blend(cv, fs, cv, rect, chans)
    exp = [cv.download(c) for c in range(4)]
    ic = host.DeviceCanvas.fromArrays(ctx, [ints])
    ic.cast(0, 12)
    exp_cast = ic.download(0)
    for s_ in (cv, fs, ic):
        s_.release()
    handle = vm.fn("create", i64, i32)(vm.env, None, 0)
    assert handle and vm.pending() is None
    self_ = vm.lib.fj_self(handle)
    create = vm.fn("canvasCreate", i32, i32, i32, vp)
    destroy = vm.fn("canvasDestroy", None, i32)
    describe = vm.fn("canvasDescribe", vp, i32)
    clone = vm.fn("canvasClone", i32, i32)
    upload = vm.fn("canvasUpload", None, i32, i32, vp, i32)
    download = vm.fn("canvasDownload", i32, i32, i32, vp)
    from_planes = vm.fn("canvasFromPlanes", i32, vp)
    cast = vm.fn("canvasCast", None, i32, i32, i32)
    blend = vm.fn("canvasBlend", None, vp)
    to_planes = vm.fn("canvasToPlanes", None, i32)
    check = vm.fn("canvasBlendCheck", None, vp, vp, vp, vp)
    planes_download = vm.fn("planesDownload", None, vp, vp, vp)
    try:
        c_id = create(vm.env, self_, h, w, vm.ints([0, 0, 0, 0]))
        f_id = create(vm.env, self_, fh, fw, vm.ints([0, 0, 0, 0]))
        assert vm.pending() is None and c_id >= 0 and f_id >= 0 and c_id != f_id
        for c in range(4):
            upload(vm.env, self_, c_id, c, vm.direct(canvas[c]), 0)
            upload(vm.env, self_, f_id, c, vm.direct(frame[c]), 0)
            assert vm.pending() is None, vm.pending()
        assert list(_ints_of(vm, describe(vm.env, self_, c_id))) == [4, h, w, 0, 0, 0, 0]
        snap = clone(vm.env, self_, c_id)
        assert vm.pending() is None and snap not in (c_id, f_id)
        desc = [c_id, f_id, c_id, 4] + rect + [v for ch in chans for v in ch]
        check(vm.env, None, vm.ints(desc), vm.ints([4, h, w, 0, 0, 0, 0]), vm.ints([4, fh, fw, 0, 0, 0, 0]), vm.ints([4, h, w, 0, 0, 0, 0]))
        assert vm.pending() is None, vm.pending()
        blend(vm.env, self_, vm.ints(desc))
        assert vm.pending() is None, vm.pending()
        out = np.zeros((h, w), np.float32)
        for c in range(4):
            assert download(vm.env, self_, c_id, c, vm.direct(out)) == 0 and vm.pending() is None
            assert np.array_equal(out.view(np.uint32), exp[c].view(np.uint32)), c
            assert download(vm.env, self_, snap, c, vm.direct(out)) == 0 and vm.pending() is None
            assert np.array_equal(out.view(np.uint32), canvas[c].view(np.uint32)), c
        # the set becomes the resident planes, and those a new set with an int32 extra plane
        to_planes(vm.env, self_, c_id)
        assert vm.pending() is None, vm.pending()
        got = [np.zeros((h, w), np.float32) for _ in range(3)]
        planes_download(vm.env, self_, vm.direct(got[0]), vm.direct(got[1]), vm.direct(got[2]))
        assert vm.pending() is None and all(np.array_equal(got[c].view(np.uint32), exp[c].view(np.uint32)) for c in range(3))
        p_id = from_planes(vm.env, self_, vm.ints([1]))
        assert vm.pending() is None and list(_ints_of(vm, describe(vm.env, self_, p_id))) == [4, h, w, 0, 0, 0, 1]
        upload(vm.env, self_, p_id, 3, vm.direct(ints), 1)
        cast(vm.env, self_, p_id, 3, 12)
        assert vm.pending() is None, vm.pending()
        assert download(vm.env, self_, p_id, 3, vm.direct(out)) == 0 and np.array_equal(out.view(np.uint32), exp_cast.view(np.uint32))
        assert download(vm.env, self_, p_id, 1, vm.direct(out)) == 0 and np.array_equal(out.view(np.uint32), exp[1].view(np.uint32))
        # capacity errors: a transfer buffer one sample short, a missing one; the plane is untouched
        before = out.copy()
        upload(vm.env, self_, c_id, 0, vm.direct(canvas[0], canvas[0].nbytes - 4), 0)
        assert vm.take()[0] == "java/lang/IllegalArgumentException"
        upload(vm.env, self_, c_id, 0, None, 0)
        assert vm.take()[0] == "java/lang/IllegalArgumentException"
        assert download(vm.env, self_, p_id, 1, vm.direct(out, out.nbytes - 1)) == -1
        assert vm.take()[0] == "java/lang/IllegalArgumentException" and np.array_equal(out, before)
        # short arrays, counts out of range
        blend(vm.env, self_, vm.ints(desc[:-1]))
        assert vm.take()[0] == "java/lang/IllegalArgumentException"
        blend(vm.env, self_, vm.ints(desc[:3] + [17] + desc[4:]))
        assert vm.take()[0] == "java/lang/IllegalArgumentException"
        assert create(vm.env, self_, h, w, vm.ints([0] * 17)) == -1
        assert vm.take()[0] == "java/lang/UnsupportedOperationException"
        # the library's own refusals come through as the same classes
        blend(vm.env, self_, vm.ints(desc[:4] + [fh, fw, 4, 5, 0, 0, 3, 5] + desc[12:]))
        assert vm.take()[0] == "java/lang/UnsupportedOperationException"
        check(vm.env, None, vm.ints(desc[:12] + [0, 7, he, 3, 3] + desc[17:]), vm.ints([4, h, w, 0, 0, 0, 0]), vm.ints([4, fh, fw, 0, 0, 0, 0]),
              vm.ints([4, h, w, 0, 0, 0, 0]))
        assert vm.take()[0] == "com/traneptora/jxlatte/io/InvalidBitstreamException"
        download(vm.env, self_, 99, 0, vm.direct(out))
        assert vm.take()[0] == "java/lang/IllegalArgumentException"
        cast(vm.env, self_, p_id, 3, 12)  # a float plane now: nothing happens
        assert vm.pending() is None
        destroy(vm.env, self_, snap)
        assert vm.pending() is None
        destroy(vm.env, self_, snap)
        assert vm.take()[0] == "java/lang/IllegalArgumentException"
        fresh = vm.fn("create", i64, i32)(vm.env, None, 0)
        assert from_planes(vm.env, vm.lib.fj_self(fresh), None) == -1
        assert vm.take()[0] == "java/lang/IllegalStateException"
        vm.fn("destroy", None, i64)(vm.env, None, fresh)
    finally:
        vm.fn("destroy", None, i64)(vm.env, None, handle)
