"""The PNG-sample natives of integration/jni/jxlatte_amd_jni.c (stagePngSamples, planesPngSamples, planesColorPeak, planesOrient),
called through ctypes over tests/stubs/fake_jni.c as tests/test_jni_shim.py calls the others: they equal the C-ABI results, and
their size checks arrive as the Java exception classes."""
import ctypes as C

import numpy as np
import pytest

from test_jni_shim import FakeJVM, _build


@pytest.mark.gpu
def test_png_sample_entries_over_jni_equal_the_c_abi(ctx, tmp_path):
    from jxlatte_amd import abi, host
    vm = FakeJVM(_build(tmp_path))
    i32, i64, vp, f32 = C.c_int32, C.c_int64, C.c_void_p, C.c_float
    rng = np.random.default_rng(77)
    h, w = 19, 23
    src = [rng.uniform(0, 1, (h, w)).astype(np.float32) for _ in range(3)]
    alpha = rng.uniform(0.1, 1, (h, w)).astype(np.float32)
    kw = dict(premultiplied=True, bitDepth=16, bigEndian=True, tfIn=abi.TF_PQ, tfOut=abi.TF_SRGB, scale=np.float32(1.25))
    exp = host.pngSamples(ctx, src, alpha, **kw)
    p = host.pngParams(src, (h, w), alpha=alpha, **kw)
    pbuf = np.frombuffer(bytes(p), np.uint8).copy()
    cbuf = np.frombuffer(bytes(p.color), np.uint8).copy()
    handle = vm.fn("create", i64, i32)(vm.env, None, 0)
    assert handle and vm.pending() is None
    self_ = vm.lib.fj_self(handle)
    stage = vm.fn("stagePngSamples", None, vp, vp, vp, vp, vp, vp)
    resident = vm.fn("planesPngSamples", None, vp, vp, vp)
    peak = vm.fn("planesColorPeak", f32, vp)
    orient = vm.fn("planesOrient", None, i32)
    upload = vm.fn("planesUpload", None, vp, vp, vp, i32, i32)
    try:
        out = np.zeros(exp.shape, exp.dtype)
        stage(vm.env, self_, vm.direct(src[0]), vm.direct(src[1]), vm.direct(src[2]), vm.direct(alpha), vm.direct(pbuf), vm.direct(out))
        assert vm.pending() is None, vm.pending()
        assert np.array_equal(out, exp)
        # the resident entries: planes up, the same samples; the peak; an orientation that exchanges the sides
        upload(vm.env, self_, vm.direct(src[0]), vm.direct(src[1]), vm.direct(src[2]), h, w)
        assert vm.pending() is None, vm.pending()
        out2 = np.zeros(exp.shape, exp.dtype)
        resident(vm.env, self_, vm.direct(alpha), vm.direct(pbuf), vm.direct(out2))
        assert vm.pending() is None, vm.pending()
        assert np.array_equal(out2, exp)
        got = peak(vm.env, self_, vm.direct(cbuf))
        assert vm.pending() is None and np.float32(got) == host.determinePeak(ctx, src, tfIn=abi.TF_PQ)
        orient(vm.env, self_, 6)
        assert vm.pending() is None, vm.pending()
        resident(vm.env, self_, vm.direct(alpha), vm.direct(pbuf), vm.direct(out2))  # the planes are w x h now
        assert vm.take()[0] == "java/lang/IllegalArgumentException"
        # size checks: an output one byte short, a short colour plane, a short alpha plane, a short parameter block
        before = out.copy()
        stage(vm.env, self_, vm.direct(src[0]), vm.direct(src[1]), vm.direct(src[2]), vm.direct(alpha), vm.direct(pbuf), vm.direct(out, out.nbytes - 1))
        assert vm.take()[0] == "java/lang/IllegalArgumentException" and np.array_equal(out, before)
        stage(vm.env, self_, vm.direct(src[0]), vm.direct(src[1], src[1].nbytes - 4), vm.direct(src[2]), vm.direct(alpha), vm.direct(pbuf), vm.direct(out))
        assert vm.take()[0] == "java/lang/IllegalArgumentException"
        stage(vm.env, self_, vm.direct(src[0]), vm.direct(src[1]), vm.direct(src[2]), vm.direct(alpha, 8), vm.direct(pbuf), vm.direct(out))
        assert vm.take()[0] == "java/lang/IllegalArgumentException"
        stage(vm.env, self_, vm.direct(src[0]), vm.direct(src[1]), vm.direct(src[2]), vm.direct(alpha), vm.direct(pbuf, pbuf.nbytes - 4), vm.direct(out))
        assert vm.take()[0] == "java/lang/IllegalArgumentException"
        fresh = vm.fn("create", i64, i32)(vm.env, None, 0)
        orient(vm.env, vm.lib.fj_self(fresh), 3)
        assert vm.take()[0] == "java/lang/IllegalStateException"
        vm.fn("destroy", None, i64)(vm.env, None, fresh)
    finally:
        vm.fn("destroy", None, i64)(vm.env, None, handle)
