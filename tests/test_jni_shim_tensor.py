"""The tensor natives of integration/jni/jxlatte_amd_jni.c (stageTensorSamples, planesTensorSamples, canvasTensorSamples), called
through ctypes over tests/stubs/fake_jni.c as tests/test_jni_shim.py calls the others: they write the tensors the C ABI writes,
their size checks arrive as the Java exception classes, and the library's own refusal of a host address comes through as one."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_jni_shim import FakeJVM, _build


@pytest.mark.gpu
def test_tensor_entries_over_jni_equal_the_c_abi(ctx, tmp_path):
    from jxlatte_amd import abi, host
    vm = FakeJVM(_build(tmp_path))
    i32, i64, vp = C.c_int32, C.c_int64, C.c_void_p
    rng = np.random.default_rng(79)
    h, w = 19, 23
    dev = "cuda:%d" % ctx.device
    src = [rng.uniform(0, 1, (h, w)).astype(np.float32) for _ in range(3)]
    alpha = rng.uniform(0.1, 1, (h, w)).astype(np.float32)
    kw = dict(premultiplied=True, writeAlpha=True, dtype="bfloat16", layout="CHW", tfIn=abi.TF_PQ, tfOut=abi.TF_SRGB, scale=np.float32(1.25),
              mean=[0.5, 0.4, 0.3, 0.2], invStd=[2.0, 3.0, 4.0, 5.0])
    exp = torch.empty((4, h, w), dtype=torch.bfloat16, device=dev)
    p = host.tensorSamples(ctx, src, alpha, exp.data_ptr(), **kw)
    pbuf = np.frombuffer(bytes(p), np.uint8).copy()
    handle = vm.fn("create", i64, i32)(vm.env, None, 0)
    assert handle and vm.pending() is None
    self_ = vm.lib.fj_self(handle)
    stage = vm.fn("stageTensorSamples", None, vp, vp, vp, vp, vp, i64)
    resident = vm.fn("planesTensorSamples", None, vp, vp, i64)
    on_set = vm.fn("canvasTensorSamples", None, i32, i32, vp, i64)
    upload = vm.fn("planesUpload", None, vp, vp, vp, i32, i32)
    create = vm.fn("canvasCreate", i32, i32, i32, vp)
    put = vm.fn("canvasUpload", None, i32, i32, vp, i32)

    def fresh():
        return torch.full((4, h, w), -3.0, dtype=torch.bfloat16, device=dev)
    try:
        out = fresh()
        stage(vm.env, self_, vm.direct(src[0]), vm.direct(src[1]), vm.direct(src[2]), vm.direct(alpha), vm.direct(pbuf), out.data_ptr())
        assert vm.pending() is None, vm.pending()
        assert torch.equal(out.view(torch.int16), exp.view(torch.int16))
        upload(vm.env, self_, vm.direct(src[0]), vm.direct(src[1]), vm.direct(src[2]), h, w)
        assert vm.pending() is None, vm.pending()
        out = fresh()
        resident(vm.env, self_, vm.direct(alpha), vm.direct(pbuf), out.data_ptr())
        assert vm.pending() is None, vm.pending()
        assert torch.equal(out.view(torch.int16), exp.view(torch.int16))
        id_ = create(vm.env, self_, h, w, vm.ints([abi.PLANE_FLOAT] * 4))
        assert vm.pending() is None, vm.pending()
        for k, a in enumerate(src + [alpha]):
            put(vm.env, self_, id_, k, vm.direct(a), abi.PLANE_FLOAT)
            assert vm.pending() is None, vm.pending()
        out = fresh()
        on_set(vm.env, self_, id_, 3, vm.direct(pbuf), out.data_ptr())
        assert vm.pending() is None, vm.pending()
        assert torch.equal(out.view(torch.int16), exp.view(torch.int16))
        # size checks of the shim: a short colour plane, a short alpha plane, a short parameter block, a missing first plane
        out = fresh()
        before = out.clone()
        stage(vm.env, self_, vm.direct(src[0]), vm.direct(src[1], src[1].nbytes - 4), vm.direct(src[2]), vm.direct(alpha), vm.direct(pbuf), out.data_ptr())
        assert vm.take()[0] == "java/lang/IllegalArgumentException"
        stage(vm.env, self_, vm.direct(src[0]), vm.direct(src[1]), vm.direct(src[2]), vm.direct(alpha, 8), vm.direct(pbuf), out.data_ptr())
        assert vm.take()[0] == "java/lang/IllegalArgumentException"
        stage(vm.env, self_, vm.direct(src[0]), vm.direct(src[1]), vm.direct(src[2]), vm.direct(alpha), vm.direct(pbuf, pbuf.nbytes - 4), out.data_ptr())
        assert vm.take()[0] == "java/lang/IllegalArgumentException"
        stage(vm.env, self_, None, vm.direct(src[1]), vm.direct(src[2]), vm.direct(alpha), vm.direct(pbuf), out.data_ptr())
        assert vm.take()[0] == "java/lang/IllegalArgumentException"
        resident(vm.env, self_, vm.direct(alpha, 8), vm.direct(pbuf), out.data_ptr())
        assert vm.take()[0] == "java/lang/IllegalArgumentException"
        # the library's refusals come through as the same class: a host address, a null address, a plane the set has not
        host_out = np.full(4 * h * w, 0x5A5A, np.uint16)
        stage(vm.env, self_, vm.direct(src[0]), vm.direct(src[1]), vm.direct(src[2]), vm.direct(alpha), vm.direct(pbuf), host_out.ctypes.data)
        assert vm.take()[0] == "java/lang/IllegalArgumentException" and np.all(host_out == 0x5A5A)
        stage(vm.env, self_, vm.direct(src[0]), vm.direct(src[1]), vm.direct(src[2]), vm.direct(alpha), vm.direct(pbuf), 0)
        assert vm.take()[0] == "java/lang/IllegalArgumentException"
        on_set(vm.env, self_, id_, 4, vm.direct(pbuf), out.data_ptr())
        assert vm.take()[0] == "java/lang/IllegalArgumentException"
        assert torch.equal(out.view(torch.int16), before.view(torch.int16))
        other = vm.fn("create", i64, i32)(vm.env, None, 0)
        resident(vm.env, vm.lib.fj_self(other), vm.direct(alpha), vm.direct(pbuf), out.data_ptr())
        assert vm.take()[0] == "java/lang/IllegalStateException"
        vm.fn("destroy", None, i64)(vm.env, None, other)
    finally:
        vm.fn("destroy", None, i64)(vm.env, None, handle)
