"""The resized tensor natives of integration/jni/jxlatte_amd_jni.c (stageTensorResized, planesTensorResized, canvasTensorResized),
called through ctypes over tests/stubs/fake_jni.c as tests/test_jni_shim_tensor.py calls their siblings: they write the tensors the
C ABI writes, their size checks arrive as the Java exception classes, and the library's own refusals come through as one."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_jni_shim import FakeJVM, _build


@pytest.mark.gpu
def test_resized_entries_over_jni_equal_the_c_abi(ctx, tmp_path):
    from jxlatte_amd import abi, host
    vm = FakeJVM(_build(tmp_path))
    i32, i64, vp = C.c_int32, C.c_int64, C.c_void_p
    rng = np.random.default_rng(80)
    h, w = 19, 23
    size, box = (6, 5), (2, 1, 20, 17)
    dev = "cuda:%d" % ctx.device
    src = [rng.uniform(0, 1, (h, w)).astype(np.float32) for _ in range(3)]
    alpha = rng.uniform(0.1, 1, (h, w)).astype(np.float32)
    kw = dict(premultiplied=True, writeAlpha=True, dtype="bfloat16", layout="CHW", tfIn=abi.TF_PQ, tfOut=abi.TF_SRGB, scale=np.float32(1.25),
              mean=[0.5, 0.4, 0.3, 0.2], invStd=[2.0, 3.0, 4.0, 5.0])
    exp = torch.empty((4,) + size, dtype=torch.bfloat16, device=dev)
    p, r = host.tensorResized(ctx, src, alpha, exp.data_ptr(), size, box, "triangle", **kw)
    pbuf = np.frombuffer(bytes(p), np.uint8).copy()
    rbuf = np.frombuffer(bytes(r), np.uint8).copy()
    handle = vm.fn("create", i64, i32)(vm.env, None, 0)
    assert handle and vm.pending() is None
    self_ = vm.lib.fj_self(handle)
    stage = vm.fn("stageTensorResized", None, vp, vp, vp, vp, vp, vp, i64)
    resident = vm.fn("planesTensorResized", None, vp, vp, vp, i64)
    on_set = vm.fn("canvasTensorResized", None, i32, i32, vp, vp, i64)
    upload = vm.fn("planesUpload", None, vp, vp, vp, i32, i32)
    create = vm.fn("canvasCreate", i32, i32, i32, vp)
    put = vm.fn("canvasUpload", None, i32, i32, vp, i32)

    def fresh():
        return torch.full((4,) + size, -3.0, dtype=torch.bfloat16, device=dev)

    def planes():
        return vm.direct(src[0]), vm.direct(src[1]), vm.direct(src[2])
    try:
        out = fresh()
        stage(vm.env, self_, *planes(), vm.direct(alpha), vm.direct(pbuf), vm.direct(rbuf), out.data_ptr())
        assert vm.pending() is None, vm.pending()
        assert torch.equal(out.view(torch.int16), exp.view(torch.int16))
        upload(vm.env, self_, *planes(), h, w)
        assert vm.pending() is None, vm.pending()
        out = fresh()
        resident(vm.env, self_, vm.direct(alpha), vm.direct(pbuf), vm.direct(rbuf), out.data_ptr())
        assert vm.pending() is None, vm.pending()
        assert torch.equal(out.view(torch.int16), exp.view(torch.int16))
        id_ = create(vm.env, self_, h, w, vm.ints([abi.PLANE_FLOAT] * 4))
        assert vm.pending() is None, vm.pending()
        for k, a in enumerate(src + [alpha]):
            put(vm.env, self_, id_, k, vm.direct(a), abi.PLANE_FLOAT)
            assert vm.pending() is None, vm.pending()
        out = fresh()
        on_set(vm.env, self_, id_, 3, vm.direct(pbuf), vm.direct(rbuf), out.data_ptr())
        assert vm.pending() is None, vm.pending()
        assert torch.equal(out.view(torch.int16), exp.view(torch.int16))
        # size checks of the shim: short planes, short parameter blocks, missing buffers, sizes below 1
        out = fresh()
        before = out.clone()
        p0, p1, p2 = planes()
        stage(vm.env, self_, p0, vm.direct(src[1], src[1].nbytes - 4), p2, vm.direct(alpha), vm.direct(pbuf), vm.direct(rbuf), out.data_ptr())
        assert vm.take()[0] == "java/lang/IllegalArgumentException"
        stage(vm.env, self_, *planes(), vm.direct(alpha, 8), vm.direct(pbuf), vm.direct(rbuf), out.data_ptr())
        assert vm.take()[0] == "java/lang/IllegalArgumentException"
        stage(vm.env, self_, *planes(), vm.direct(alpha), vm.direct(pbuf, pbuf.nbytes - 4), vm.direct(rbuf), out.data_ptr())
        assert vm.take()[0] == "java/lang/IllegalArgumentException"
        stage(vm.env, self_, *planes(), vm.direct(alpha), vm.direct(pbuf), vm.direct(rbuf, rbuf.nbytes - 4), out.data_ptr())
        assert vm.take()[0] == "java/lang/IllegalArgumentException"
        stage(vm.env, self_, *planes(), vm.direct(alpha), vm.direct(pbuf), None, out.data_ptr())
        assert vm.take()[0] == "java/lang/IllegalArgumentException"
        stage(vm.env, self_, None, p1, p2, vm.direct(alpha), vm.direct(pbuf), vm.direct(rbuf), out.data_ptr())
        assert vm.take()[0] == "java/lang/IllegalArgumentException"
        resident(vm.env, self_, vm.direct(alpha, 8), vm.direct(pbuf), vm.direct(rbuf), out.data_ptr())
        assert vm.take()[0] == "java/lang/IllegalArgumentException"
        zero = np.frombuffer(bytes(host.resizeParams((h, w), (0, 5))), np.uint8).copy()
        on_set(vm.env, self_, id_, 3, vm.direct(pbuf), vm.direct(zero), out.data_ptr())
        assert vm.take()[0] == "java/lang/IllegalArgumentException"
        # the library's refusals come through as the same class: a host address, a box outside the image, an unknown filter
        host_out = np.full(4 * size[0] * size[1], 0x5A5A, np.uint16)
        stage(vm.env, self_, *planes(), vm.direct(alpha), vm.direct(pbuf), vm.direct(rbuf), host_out.ctypes.data)
        assert vm.take()[0] == "java/lang/IllegalArgumentException" and np.all(host_out == 0x5A5A)
        for bad in (host.resizeParams((h, w), size, (10, 1, 20, 17)), host.resizeParams((h, w), size, box, 7)):
            bbuf = np.frombuffer(bytes(bad), np.uint8).copy()
            stage(vm.env, self_, *planes(), vm.direct(alpha), vm.direct(pbuf), vm.direct(bbuf), out.data_ptr())
            assert vm.take()[0] == "java/lang/IllegalArgumentException"
        on_set(vm.env, self_, id_, 4, vm.direct(pbuf), vm.direct(rbuf), out.data_ptr())
        assert vm.take()[0] == "java/lang/IllegalArgumentException"
        assert torch.equal(out.view(torch.int16), before.view(torch.int16))
        other = vm.fn("create", i64, i32)(vm.env, None, 0)
        resident(vm.env, vm.lib.fj_self(other), vm.direct(alpha), vm.direct(pbuf), vm.direct(rbuf), out.data_ptr())
        assert vm.take()[0] == "java/lang/IllegalStateException"
        vm.fn("destroy", None, i64)(vm.env, None, other)
    finally:
        vm.fn("destroy", None, i64)(vm.env, None, handle)
