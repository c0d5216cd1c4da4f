"""The patch natives of integration/jni/jxlatte_amd_jni.c (patchBins, stagePatches, planesPatches), called through ctypes over
tests/stubs/fake_jni.c as tests/test_jni_shim_splines.py calls the spline natives: they equal the C-ABI results, and their
argument checks and the reference's three errors arrive as the Java exception classes."""
import ctypes as C

import numpy as np
import pytest

import patch_ref as R
from test_jni_shim import FakeJVM, _build

F = np.float32


def _objects(vm, items):
    vm.lib.fj_objects.restype, vm.lib.fj_objects.argtypes = C.c_void_p, [C.c_int64]
    vm.lib.fj_set_object.restype, vm.lib.fj_set_object.argtypes = None, [C.c_void_p, C.c_int64, C.c_void_p]
    arr = vm.lib.fj_objects(len(items))
    for i, a in enumerate(items):
        vm.lib.fj_set_object(arr, i, vm.direct(a))
    return arr


def _stage():
    info = R.make_info(1)
    rng = np.random.default_rng(3)
    h, w = 40, 70
    frame = [rng.uniform(0, 1, (h, w)).astype(F) for _ in range(3)] + [rng.uniform(0.1, 0.9, (h, w)).astype(F)]
    ref = [rng.uniform(0, 1, (20, 30)).astype(F) for _ in range(3)] + [rng.uniform(0.1, 0.9, (20, 30)).astype(F)]
    rows = [[[3, 0, 1], [3, 0, 0]], [[2, 0, 0], [0, 0, 0]]]
    patches = [R.patch(0, 1, 2, 12, 20, [(0, 0), (5, 9), (28, 50)], [rows[0], rows[1], rows[0]]), R.patch(2, 0, 0, 99, 99, [(0, 0)], [rows[1]])]
    pos, blend = R.pos_table(info, patches)
    return info, frame, [ref, None, None, None], pos, blend


def test_patch_bins_over_jni_equals_the_c_abi(tmp_path):
    from jxlatte_amd import host
    vm = FakeJVM(_build(tmp_path))
    i32, vp = C.c_int32, C.c_void_p
    info, frame, ref, pos, blend = _stage()
    bins = vm.fn("patchBins", vp, i32, i32, vp, vp, vp, vp, i32, vp, vp, vp)
    shape = [20, 30, 0, 0, 0, 0, 0, 0]
    ftype, rtype = [0] * 4, [0] * 4 + [-1] * 12
    words = pos.view(np.int32).reshape(-1)
    arr = bins(vm.env, None, 40, 70, vm.ints(ftype), vm.ints(rtype), vm.ints(words), vm.ints(blend), 3, vm.ints([1]), vm.ints([0]), vm.ints(shape))
    assert vm.pending() is None and arr, vm.pending()
    tile, start, lst = host.patch_bins(pos, blend, 3, [True], [False], 40, 70, ftype, [(20, 30), None, None, None], rtype)
    got = np.ctypeslib.as_array(C.cast(vm.lib.fj_data(arr), C.POINTER(C.c_int32)), shape=(vm.lib.fj_length(arr),))
    assert list(got) == [len(tile), len(lst)] + list(tile) + list(start) + list(lst)
    bad = pos.copy()
    bad["y0"][1] = 30  # 30 + 12 > 40
    bins(vm.env, None, 40, 70, vm.ints(ftype), vm.ints(rtype), vm.ints(bad.view(np.int32).reshape(-1)), vm.ints(blend), 3, vm.ints([1]), vm.ints([0]), vm.ints(shape))
    cls, msg = vm.take()
    assert cls == "com/traneptora/jxlatte/io/InvalidBitstreamException" and msg == "Patch size out of bounds"
    bins(vm.env, None, 40, 70, vm.ints(ftype), vm.ints(rtype), vm.ints(words[:-1]), vm.ints(blend), 3, vm.ints([1]), vm.ints([0]), vm.ints(shape))
    assert vm.take()[0] == "java/lang/IllegalArgumentException"
    bins(vm.env, None, 40, 70, vm.ints(ftype), vm.ints(rtype[:-1]), vm.ints(words), vm.ints(blend), 3, vm.ints([1]), vm.ints([0]), vm.ints(shape))
    assert vm.take()[0] == "java/lang/IllegalArgumentException"
    bins(vm.env, None, 40, 70, vm.ints(ftype), vm.ints(rtype), None, vm.ints(blend), 3, vm.ints([1]), vm.ints([0]), vm.ints(shape))
    assert vm.take()[0] == "java/lang/IllegalArgumentException"


@pytest.mark.gpu
def test_patch_entries_over_jni_equal_the_c_abi(ctx, tmp_path):
    from jxlatte_amd import host
    vm = FakeJVM(_build(tmp_path))
    i32, i64, vp = C.c_int32, C.c_int64, C.c_void_p
    info, frame, ref, pos, blend = _stage()
    h, w = frame[0].shape
    exp = host.computePatches(ctx, [b.copy() for b in frame], ref, pos, blend, 3, [True], [False])
    handle = vm.fn("create", i64, i32)(vm.env, None, 0)
    assert handle and vm.pending() is None
    self_ = vm.lib.fj_self(handle)
    stage = vm.fn("stagePatches", None, vp, vp, i32, i32, vp, vp, vp, vp, i32, vp, vp, vp)
    resident = vm.fn("planesPatches", None, vp, vp, vp, vp, vp, vp, vp, vp, vp)
    upload = vm.fn("planesUpload", None, vp, vp, vp, i32, i32)
    download = vm.fn("planesDownload", None, vp, vp, vp)
    shape, words = [20, 30, 0, 0, 0, 0, 0, 0], pos.view(np.int32).reshape(-1)
    ftype, rtype = [0] * 4, [0] * 4 + [-1] * 12
    refs = _objects(vm, list(ref[0]) + [None] * 12)
    try:
        out = [b.copy() for b in frame]
        stage(vm.env, self_, _objects(vm, out), vm.ints(ftype), h, w, refs, vm.ints(rtype), vm.ints(words), vm.ints(blend), 3, vm.ints([1]), vm.ints([0]),
              vm.ints(shape))
        assert vm.pending() is None, vm.pending()
        assert all(R.same_bits(a, b) for a, b in zip(out, exp))
        src = [b.copy() for b in frame]
        upload(vm.env, self_, vm.direct(src[0]), vm.direct(src[1]), vm.direct(src[2]), h, w)
        assert vm.pending() is None, vm.pending()
        resident(vm.env, self_, _objects(vm, src[3:]), vm.ints([0]), refs, vm.ints(rtype), vm.ints(words), vm.ints(blend), vm.ints([1]), vm.ints([0]), vm.ints(shape))
        assert vm.pending() is None, vm.pending()
        got = [np.zeros((h, w), F) for _ in range(3)]
        download(vm.env, self_, vm.direct(got[0]), vm.direct(got[1]), vm.direct(got[2]))
        assert vm.pending() is None, vm.pending()
        assert all(R.same_bits(a, b) for a, b in zip(got + src[3:], exp))
        # argument checks: a frame plane buffer too small, a missing frame plane, a typed reference plane too small, no resident planes
        small = _objects(vm, out)
        vm.lib.fj_set_object(small, 1, vm.direct(out[1], out[1].nbytes - 4))
        stage(vm.env, self_, small, vm.ints(ftype), h, w, refs, vm.ints(rtype), vm.ints(words), vm.ints(blend), 3, vm.ints([1]), vm.ints([0]), vm.ints(shape))
        assert vm.take()[0] == "java/lang/IllegalArgumentException"
        stage(vm.env, self_, _objects(vm, out[:3] + [None]), vm.ints(ftype), h, w, refs, vm.ints(rtype), vm.ints(words), vm.ints(blend), 3, vm.ints([1]),
              vm.ints([0]), vm.ints(shape))
        assert vm.take()[0] == "java/lang/IllegalArgumentException"
        stage(vm.env, self_, _objects(vm, out), vm.ints(ftype), h, w, refs, vm.ints(rtype), vm.ints(words), vm.ints(blend), 3, vm.ints([1]), vm.ints([0]),
              vm.ints([21, 30, 0, 0, 0, 0, 0, 0]))
        assert vm.take()[0] == "java/lang/IllegalArgumentException"
        fresh = vm.fn("create", i64, i32)(vm.env, None, 0)
        resident(vm.env, vm.lib.fj_self(fresh), _objects(vm, src[3:]), vm.ints([0]), refs, vm.ints(rtype), vm.ints(words), vm.ints(blend), vm.ints([1]),
                 vm.ints([0]), vm.ints(shape))
        assert vm.take()[0] == "java/lang/IllegalStateException"
        vm.fn("destroy", None, i64)(vm.env, None, fresh)
    finally:
        vm.fn("destroy", None, i64)(vm.env, None, handle)
