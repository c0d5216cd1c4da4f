"""The batch native of integration/jni/jxlatte_amd_jni.c (tensorResizedBatch), called through ctypes over tests/stubs/fake_jni.c as
tests/test_jni_shim_tensor_resized.py calls its siblings: it writes the batch the C ABI writes, its size checks arrive as the
Java exception classes, and the library's own refusals come through as one."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_jni_shim import FakeJVM, _build


def _longs(vm, values):
    a = np.ascontiguousarray(values, np.int64)
    vm.keep.append(a)
    return vm.lib.fj_longs(a.ctypes.data, a.size)


@pytest.mark.gpu
def test_batch_native_over_jni_equals_the_c_abi(ctx, tmp_path):
    from jxlatte_amd import abi, host
    vm = FakeJVM(_build(tmp_path))
    i32, i64, vp = C.c_int32, C.c_int64, C.c_void_p
    rng = np.random.default_rng(81)
    dev = "cuda:%d" % ctx.device
    size = (6, 5)
    shapes = [(19, 23), (5, 7), (19, 23)]
    # the host planes of all items in one buffer: per item three colour planes and an alpha plane
    sizes = [4 * h * w for h, w in shapes]
    starts = np.concatenate([[0], np.cumsum([4 * s for s in sizes])]).astype(np.int64)
    pool = np.empty(int(starts[-1]), np.uint8)
    planes, alphas = [], []
    for k, (h, w) in enumerate(shapes):
        view = pool[starts[k]:starts[k + 1]].view(np.float32).reshape(4, h, w)
        view[:3] = rng.uniform(0, 1, (3, h, w)).astype(np.float32)
        view[3] = rng.uniform(0.1, 1, (h, w)).astype(np.float32)
        planes.append([view[0], view[1], view[2]])
        alphas.append(view[3])
    kw = dict(premultiplied=True, writeAlpha=True, dtype="bfloat16", layout="CHW", tfIn=abi.TF_PQ, tfOut=abi.TF_SRGB, scale=np.float32(1.25))
    boxes = [(2, 1, 20, 17), None, None]
    filters = ["triangle", "box", "triangle"]
    items = [host.tensorBatchItem(size, boxes[k], filters[k], planes=planes[k], alpha=alphas[k], **kw) for k in range(3)]
    # the third item from a plane set of the same context
    handle = vm.fn("create", i64, i32)(vm.env, None, 0)
    assert handle and vm.pending() is None
    self_ = vm.lib.fj_self(handle)
    native = vm.fn("tensorResizedBatch", None, vp, vp, vp, vp, vp, i64)
    create = vm.fn("canvasCreate", i32, i32, i32, vp)
    put = vm.fn("canvasUpload", None, i32, i32, vp, i32)
    try:
        id_ = create(vm.env, self_, 19, 23, vm.ints([abi.PLANE_FLOAT] * 4))
        assert vm.pending() is None, vm.pending()
        for k, a in enumerate(planes[2] + [alphas[2]]):
            put(vm.env, self_, id_, k, vm.direct(np.ascontiguousarray(a)), abi.PLANE_FLOAT)
            assert vm.pending() is None, vm.pending()
        # what the C ABI writes: the per-item single-image entry, through the library's own context
        exp = torch.empty((3, 4) + size, dtype=torch.bfloat16, device=dev)
        for k in range(3):
            host.tensorResized(ctx, planes[k], alphas[k], exp[k].data_ptr(), size, boxes[k], filters[k], **kw)
        heads = np.array([abi.BATCH_HOST, -1, -1, abi.BATCH_HOST, -1, -1, abi.BATCH_SET, id_, 3], np.int32)
        offs = []
        for k in range(2):
            offs += [int(starts[k]) + c * sizes[k] for c in range(4)]
        offs += [-1, -1, -1, -1]
        pbuf = np.frombuffer(b"".join(bytes(it.p) for it in items), np.uint8).copy()
        rbuf = np.frombuffer(b"".join(bytes(it.r) for it in items), np.uint8).copy()

        def fresh():
            return torch.full((3, 4) + size, -3.0, dtype=torch.bfloat16, device=dev)
        out = fresh()
        native(vm.env, self_, vm.ints(heads), vm.direct(pool), _longs(vm, offs), vm.direct(pbuf), vm.direct(rbuf), out.data_ptr())
        assert vm.pending() is None, vm.pending()
        assert torch.equal(out.view(torch.int16), exp.view(torch.int16))
        # the shim's size checks: array lengths, short parameter blocks, planes outside the buffer, sizes below 1, missing buffers
        out = fresh()
        before = out.clone()

        def refused(cls, heads=heads, pool_=vm.direct(pool), offs=offs, p=None, r=None, ptr=None):
            native(vm.env, self_, vm.ints(np.asarray(heads, np.int32)) if heads is not None else None, pool_, _longs(vm, offs) if offs is not None else None,
                   vm.direct(pbuf) if p is None else p, vm.direct(rbuf) if r is None else r, out.data_ptr() if ptr is None else ptr)
            assert vm.take()[0] == cls
        bad = "java/lang/IllegalArgumentException"
        refused(bad, heads=heads[:8])
        refused(bad, heads=heads[:0])
        refused(bad, heads=None)
        refused(bad, offs=offs[:11])
        refused(bad, offs=None)
        refused(bad, p=vm.direct(pbuf, pbuf.nbytes - 4))
        refused(bad, r=vm.direct(rbuf, rbuf.nbytes - 4))
        refused(bad, p=None, r=vm.direct(rbuf[:28]))
        refused(bad, offs=offs[:3] + [int(starts[-1]) - sizes[0] + 4] + offs[4:])  # item 0's alpha plane ends past the buffer
        refused(bad, offs=[-2] + offs[1:])
        refused(bad, pool_=vm.direct(pool, int(starts[2]) - 4))  # item 1's alpha plane is cut short
        refused(bad, pool_=None)
        zero = rbuf.copy()
        zero.view(np.int32)[7 + 4] = 0  # item 1's out_height
        refused(bad, r=vm.direct(zero))
        # the library's refusals come through as the same class: a host address, disagreeing sizes, a box outside its image, an
        # unknown set; a resident item on a context without resident planes is an IllegalStateException
        host_out = np.full(3 * 4 * size[0] * size[1], 0x5A5A, np.uint16)
        refused(bad, ptr=host_out.ctypes.data)
        assert np.all(host_out == 0x5A5A)
        other = rbuf.copy()
        other.view(np.int32)[7 + 4] = size[0] + 1
        refused(bad, r=vm.direct(other))
        outside = rbuf.copy()
        outside.view(np.int32)[0] = 10  # item 0's box_x0: 10 + 20 > 23
        refused(bad, r=vm.direct(outside))
        refused(bad, heads=list(heads[:7]) + [1 << 20, 3])
        refused("java/lang/IllegalStateException", heads=[abi.BATCH_RESIDENT, -1, -1] + list(heads[3:]), offs=[-1, -1, -1] + offs[3:])
        assert torch.equal(out.view(torch.int16), before.view(torch.int16))
    finally:
        vm.fn("destroy", None, i64)(vm.env, None, handle)
