"""The natives of integration/jni/jxlatte_amd_jni.c that patches on plane sets add (canvasCastPlanes, canvasPatches,
canvasPatchesCheck), called through ctypes over tests/stubs/fake_jni.c as tests/test_jni_shim_canvas.py calls the others: they
give the C ABI's results, and their refusals -- the library's and the shim's own size checks -- arrive as the Java exception
classes."""
import ctypes as C

import numpy as np
import pytest

from test_jni_shim import FakeJVM, _build


def _slot(n, h=0, w=0, types=()):
    """one slot of canvasPatchesCheck's `refs`: {n, h, w, type[16]}"""
    return [n, h, w] + list(types) + [0] * (16 - len(types))


@pytest.mark.gpu
def test_patch_set_entries_over_jni_equal_the_c_abi(ctx, tmp_path):
    from conftest import assert_bits_equal
    from jxlatte_amd import abi, host
    vm = FakeJVM(_build(tmp_path))
    i32, i64, vp = C.c_int32, C.c_int64, C.c_void_p
    rng = np.random.default_rng(71)
    h, w, rh, rw = 21, 37, 12, 18
    frame = [rng.integers(0, 256, (h, w)).astype(np.int32) for _ in range(4)]
    ref = [rng.integers(0, 256, (rh, rw)).astype(np.int32) for _ in range(4)]
    pos = np.array([(2, 3, 8, 9, 0, 1, 2, 0), (10, 20, 8, 9, 0, 3, 4, 0), (12, 25, 5, 5, 2, 0, 0, 0)], abi.PATCH_POS_DTYPE)
    blend = np.array([[[2, 0, 1]] * 4], np.int32)  # patch mode 2 = blendAdd; float planes after the hoisted casts
    # the C ABI on the session's context
    fs, rs = host.DeviceCanvas.fromArrays(ctx, frame), host.DeviceCanvas.fromArrays(ctx, ref)
    host.canvas_cast_planes(ctx, [(fs, n, 8) for n in range(4)] + [(rs, n, 8) for n in range(4)])
    exp_cast = [rs.download(n) for n in range(4)]
    host.canvas_patches(fs, [rs, None, rs, None], pos, blend, 3, [True], [False])
    exp = [fs.download(n) for n in range(4)]
    fs.release()
    rs.release()
    assert exp[0].dtype == np.float32 and not np.array_equal(exp[0], frame[0].astype(np.float32) / 255)
    # the same over JNI, on a context of the shim's own
    handle = vm.fn("create", i64, i32)(vm.env, None, 0)
    assert handle and vm.pending() is None
    self_ = vm.lib.fj_self(handle)
    create = vm.fn("canvasCreate", i32, i32, i32, vp)
    upload = vm.fn("canvasUpload", None, i32, i32, vp, i32)
    download = vm.fn("canvasDownload", i32, i32, i32, vp)
    cast = vm.fn("canvasCastPlanes", None, vp)
    patches = vm.fn("canvasPatches", None, i32, i32, vp, vp, vp, i32, vp, vp)
    pos_i, blend_i, isa, assoc = vm.ints(pos.view(np.int32)), vm.ints(blend), vm.ints([1]), vm.ints([0])

    def planes_of(id_, shape, dtype):
        out = []
        for n in range(4):
            a = np.zeros(shape, dtype)
            t = download(vm.env, self_, id_, n, vm.direct(a))
            assert vm.pending() is None and t == (0 if dtype == np.float32 else 1), (vm.pending(), t)
            out.append(a)
        return out
    try:
        f_id = create(vm.env, self_, h, w, vm.ints([1] * 4))
        r_id = create(vm.env, self_, rh, rw, vm.ints([1] * 4))
        assert vm.pending() is None and f_id >= 0 and r_id >= 0 and f_id != r_id
        for n in range(4):
            upload(vm.env, self_, f_id, n, vm.direct(frame[n]), 1)
            upload(vm.env, self_, r_id, n, vm.direct(ref[n]), 1)
        assert vm.pending() is None, vm.pending()
        # refusals first: nothing is queued and no tag changes
        cast(vm.env, self_, vm.ints([f_id, 0, 8, f_id, 0, 8]))
        assert vm.take() == ("java/lang/IllegalArgumentException", "canvas cast: a plane is named twice")
        cast(vm.env, self_, vm.ints([f_id, 0, 8, r_id, 1, 0]))
        assert vm.take() == ("java/lang/IllegalArgumentException", "invalid Max Value")
        cast(vm.env, self_, vm.ints([f_id, 0, 8, f_id]))
        assert vm.take()[0] == "java/lang/IllegalArgumentException"   # the shim's: 3 ints per item
        cast(vm.env, self_, vm.ints([f_id, 0, 8] * 81))
        assert vm.take()[0] == "java/lang/IllegalArgumentException"   # the shim's: more than 80 planes
        cast(vm.env, self_, None)
        assert vm.take()[0] == "java/lang/IllegalArgumentException"
        for n, a in enumerate(planes_of(f_id, (h, w), np.int32)):
            assert np.array_equal(a, frame[n])
        # the casts in one call, then the patches
        cast(vm.env, self_, vm.ints([v for id_ in (f_id, r_id) for n in range(4) for v in (id_, n, 8)]))
        assert vm.pending() is None, vm.pending()
        for a, b in zip(planes_of(r_id, (rh, rw), np.float32), exp_cast):
            assert_bits_equal(a, b, "canvasCastPlanes")
        patches(vm.env, self_, f_id, 0, vm.ints([r_id, -1, r_id, -1]), pos_i, blend_i, 3, isa, assoc)
        assert vm.pending() is None, vm.pending()
        for n, (a, b) in enumerate(zip(planes_of(f_id, (h, w), np.float32), exp)):
            assert_bits_equal(a, b, "canvasPatches, plane %d" % n)
        for a, b in zip(planes_of(r_id, (rh, rw), np.float32), exp_cast):  # nothing writes a reference plane
            assert_bits_equal(a, b, "canvasPatches, reference")
        # the library's refusals as the Java classes
        patches(vm.env, self_, f_id, 0, vm.ints([r_id, -1, f_id, -1]), pos_i, blend_i, 3, isa, assoc)
        assert vm.take() == ("java/lang/IllegalArgumentException", "canvas patches: the frame set is a reference set")
        patches(vm.env, self_, f_id, 1, vm.ints([r_id, -1, r_id, -1]), pos_i, blend_i, 3, isa, assoc)
        assert vm.take() == ("java/lang/IllegalStateException", "no resident planes")
        patches(vm.env, self_, f_id, 0, vm.ints([r_id, -1, 99, -1]), pos_i, blend_i, 3, isa, assoc)
        assert vm.take() == ("java/lang/IllegalArgumentException", "canvas: unknown set")
        far = pos.copy()
        far[1]["ref_y0"] = 5
        patches(vm.env, self_, f_id, 0, vm.ints([r_id, -1, r_id, -1]), vm.ints(far.view(np.int32)), blend_i, 3, isa, assoc)
        assert vm.take() == ("com/traneptora/jxlatte/io/InvalidBitstreamException", "Patch too large")
        # ... and the shim's own checks
        patches(vm.env, self_, f_id, 0, vm.ints([r_id, -1, r_id]), pos_i, blend_i, 3, isa, assoc)
        assert vm.take()[0] == "java/lang/IllegalArgumentException"
        patches(vm.env, self_, f_id, 0, vm.ints([r_id, -1, r_id, -1]), vm.ints(pos.view(np.int32)[:-1]), blend_i, 3, isa, assoc)
        assert vm.take()[0] == "java/lang/IllegalArgumentException"
        patches(vm.env, self_, f_id, 0, vm.ints([r_id, -1, r_id, -1]), pos_i, vm.ints(blend.reshape(-1)[:-1]), 3, isa, assoc)
        assert vm.take()[0] == "java/lang/IllegalArgumentException"
        for n, (a, b) in enumerate(zip(planes_of(f_id, (h, w), np.float32), exp)):
            assert_bits_equal(a, b, "after the refusals, plane %d" % n)
    finally:
        vm.fn("destroy", None, i64)(vm.env, None, handle)


def test_patches_check_over_jni(tmp_path):
    """canvasPatchesCheck needs no device: jxl_canvas_patches_check's refusals with the library's own messages"""
    from jxlatte_amd import abi
    vm = FakeJVM(_build(tmp_path))
    i32, vp = C.c_int32, C.c_void_p
    check = vm.fn("canvasPatchesCheck", i32, vp, i32, vp, vp, vp, i32, vp, vp)
    pos = np.array([(2, 3, 8, 9, 0, 1, 2, 0), (10, 20, 8, 9, 0, 3, 4, 0), (12, 25, 5, 5, 2, 0, 0, 0)], abi.PATCH_POS_DTYPE)
    blend = np.array([[[2, 0, 1]] * 4], np.int32)
    frame = [4, 21, 37, 0, 0, 0, 0]
    small, absent, itself = _slot(4, 12, 18, [0] * 4), _slot(0), _slot(-1)

    def run(frame=frame, refs=small + absent + small + absent, pos=pos, resident=0, n_color=3):
        r = check(vm.env, None, vm.ints(frame), resident, vm.ints(refs), vm.ints(pos.view(np.int32)), vm.ints(blend), n_color, vm.ints([1]), vm.ints([0]))
        return r, vm.take()
    assert run() == (-1, None)
    assert run(resident=1, frame=[4, 21, 37, 1, 1, 1, 0]) == (-1, None)
    assert run(refs=small + absent + itself + absent)[1] == ("java/lang/IllegalArgumentException", "canvas patches: the frame set is a reference set")
    assert run(frame=[3, 21, 37, 0, 0, 0])[1] == ("java/lang/IllegalArgumentException", "canvas patches: the frame set holds one plane per channel")
    assert run(refs=small + absent + _slot(4, 12, 18, [0, 1, 0, 0]) + absent) == \
        (2, ("java/lang/IllegalArgumentException", "patches: a reference plane and its frame plane differ in type"))
    far = pos.copy()
    far[1]["x0"] = 30
    assert run(pos=far) == (1, ("com/traneptora/jxlatte/io/InvalidBitstreamException", "Patch size out of bounds"))
    # the shim's own: a short refs array, a plane count outside -1..16, no frame shape
    assert run(refs=(small + absent + small)[:-1])[1][0] == "java/lang/IllegalArgumentException"
    assert run(refs=small + absent + _slot(17) + absent)[1][0] == "java/lang/IllegalArgumentException"
    assert run(frame=[4, 21])[1][0] == "java/lang/IllegalArgumentException"
