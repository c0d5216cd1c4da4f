"""The tone-mapping native of integration/jni/jxlatte_amd_jni.c (setToneMap), called through ctypes over tests/stubs/fake_jni.c as
tests/test_jni_shim.py calls the others: armed, stageColorConvert and stagePngSamples give the C-ABI's armed results -- the PNG
entry's size check counts three channels for a one-plane image then --, null clears, and a refused block or a short buffer arrive
as IllegalArgumentException."""
import ctypes as C

import numpy as np
import pytest

import tone_map_model as tm
from test_jni_shim import FakeJVM, _build


@pytest.mark.gpu
def test_set_tone_map_over_jni_equals_the_c_abi(ctx, tmp_path):
    from jxlatte_amd import abi, host
    vm = FakeJVM(_build(tmp_path))
    i32, i64, vp = C.c_int32, C.c_int64, C.c_void_p
    v = tm.pixels(19, 23, 4)
    n = v[0].size
    block = host.toneMapParams(tm.LUM_2020, 10000.0, 1000.0, 203.0, True)
    try:
        host.setToneMap(ctx, block)
        exp = host.colorConvert(ctx, v, tfOut=abi.TF_SRGB)
        exp_grey = host.pngSamples(ctx, v[:1], tfOut=abi.TF_SRGB)
    finally:
        host.setToneMap(ctx, None)
    plain = host.colorConvert(ctx, v, tfOut=abi.TF_SRGB)
    handle = vm.fn("create", i64, i32)(vm.env, None, 0)
    assert handle and vm.pending() is None
    self_ = vm.lib.fj_self(handle)
    arm = vm.fn("setToneMap", None, vp)
    convert = vm.fn("stageColorConvert", None, vp, vp, vp, i64, vp, vp, vp, vp)
    png = vm.fn("stagePngSamples", None, vp, vp, vp, vp, vp, vp)
    cp = np.frombuffer(bytes(host.colorParams(list(v), tfOut=abi.TF_SRGB)), np.uint8).copy()
    gp = np.frombuffer(bytes(host.pngParams(v[:1], v[0].shape, tfOut=abi.TF_SRGB)), np.uint8).copy()
    tb = np.frombuffer(bytes(block), np.uint8).copy()

    def run():
        out = [np.zeros(v[0].shape, np.float32) for _ in range(3)]
        convert(vm.env, self_, vm.direct(v[0]), vm.direct(v[1]), vm.direct(v[2]), n, vm.direct(cp), vm.direct(out[0]), vm.direct(out[1]), vm.direct(out[2]))
        assert vm.pending() is None, vm.pending()
        return out
    try:
        assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(run(), plain))
        arm(vm.env, self_, vm.direct(tb))
        assert vm.pending() is None, vm.pending()
        assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(run(), exp))
        # a one-plane image gives three channels while armed: the shim's size check follows
        grey = np.zeros(exp_grey.shape, exp_grey.dtype)
        png(vm.env, self_, vm.direct(v[0]), None, None, None, vm.direct(gp), vm.direct(grey))
        assert vm.pending() is None, vm.pending()
        assert np.array_equal(grey, exp_grey)
        short = np.zeros(exp_grey.shape[:2] + (1,), exp_grey.dtype)
        png(vm.env, self_, vm.direct(v[0]), None, None, None, vm.direct(gp), vm.direct(short))
        assert vm.take()[0] == "java/lang/IllegalArgumentException" and not short.any()
        # a refused block leaves the armed one in place; a short buffer is refused by the shim
        bad = host.toneMapParams(tm.LUM_2020, 10000.0, 20000.0, 203.0, True)
        arm(vm.env, self_, vm.direct(np.frombuffer(bytes(bad), np.uint8).copy()))
        assert vm.take()[0] == "java/lang/IllegalArgumentException"
        arm(vm.env, self_, vm.direct(tb, tb.nbytes - 4))
        assert vm.take()[0] == "java/lang/IllegalArgumentException"
        assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(run(), exp))
        arm(vm.env, self_, None)  # cleared
        assert vm.pending() is None, vm.pending()
        assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(run(), plain))
        one = np.zeros(exp_grey.shape[:2] + (1,), exp_grey.dtype)
        png(vm.env, self_, vm.direct(v[0]), None, None, None, vm.direct(gp), vm.direct(one))
        assert vm.pending() is None, vm.pending()
    finally:
        vm.fn("destroy", None, i64)(vm.env, None, handle)
