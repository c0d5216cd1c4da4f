"""The varblock natives of integration/jni/jxlatte_amd_jni.c (stageVarblocks, planesVarblocks), called through ctypes over
tests/stubs/fake_jni.c as tests/test_jni_shim.py calls the others: they equal the C-ABI results, and their size checks and the
library's refusals arrive as the Java exception classes."""
import ctypes as C

import numpy as np
import pytest

import varblocks_cases
from test_jni_shim import FakeJVM, _build


@pytest.mark.gpu
def test_varblock_entries_over_jni_equal_the_c_abi(ctx, tmp_path):
    from jxlatte_amd import host
    vm = FakeJVM(_build(tmp_path))
    i32, i64, vp = C.c_int32, C.c_int64, C.c_void_p
    h, w, cells, blocks = varblocks_cases.CASES["c_21x37_ragged"]
    src = [np.ascontiguousarray(p) for p in varblocks_cases.samples("c_21x37_ragged")]
    flat = [v for b in blocks for v in b]
    n = len(blocks)
    exp = host.varblocks(ctx, np.stack(src), blocks, cells)
    handle = vm.fn("create", i64, i32)(vm.env, None, 0)
    assert handle and vm.pending() is None
    self_ = vm.lib.fj_self(handle)
    stage = vm.fn("stageVarblocks", None, vp, vp, vp, i32, i32, vp, i32, i32, i32, vp, vp, vp)
    resident = vm.fn("planesVarblocks", None, vp, i32, i32, i32)
    upload = vm.fn("planesUpload", None, vp, vp, vp, i32, i32)
    download = vm.fn("planesDownload", None, vp, vp, vp)

    def same(got):
        return all(np.array_equal(np.where(np.isnan(g), np.uint32(0x7fc00000), g.view(np.uint32)),
                                  np.where(np.isnan(e), np.uint32(0x7fc00000), e.view(np.uint32))) for g, e in zip(got, exp))
    try:
        out = [np.full((h, w), np.float32(-3.5)) for _ in range(3)]
        ins = [vm.direct(a) for a in src]
        stage(vm.env, self_, ins[0], ins[1], ins[2], h, w, vm.ints(flat), n, cells[0], cells[1], *[vm.direct(a) for a in out])
        assert vm.pending() is None, vm.pending()
        assert same(out)
        # in place: the output buffers are the input buffers
        inplace = [a.copy() for a in src]
        bufs = [vm.direct(a) for a in inplace]
        stage(vm.env, self_, bufs[0], bufs[1], bufs[2], h, w, vm.ints(flat), n, cells[0], cells[1], bufs[0], bufs[1], bufs[2])
        assert vm.pending() is None, vm.pending()
        assert same(inplace)
        # the resident entry: planes up, the map drawn, planes down
        upload(vm.env, self_, ins[0], ins[1], ins[2], h, w)
        assert vm.pending() is None, vm.pending()
        resident(vm.env, self_, vm.ints(flat), n, cells[0], cells[1])
        assert vm.pending() is None, vm.pending()
        down = [np.zeros((h, w), np.float32) for _ in range(3)]
        download(vm.env, self_, *[vm.direct(a) for a in down])
        assert vm.pending() is None, vm.pending()
        assert same(down)
        # size checks: a short plane, a missing plane, a short output, a block array shorter than 3 * nBlocks, a negative count
        before = [a.copy() for a in out]
        outs = [vm.direct(a) for a in out]

        def untouched():
            return all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(out, before))
        stage(vm.env, self_, ins[0], vm.direct(src[1], src[1].nbytes - 4), ins[2], h, w, vm.ints(flat), n, cells[0], cells[1], *outs)
        assert vm.take()[0] == "java/lang/IllegalArgumentException" and untouched()
        stage(vm.env, self_, ins[0], None, ins[2], h, w, vm.ints(flat), n, cells[0], cells[1], *outs)
        assert vm.take()[0] == "java/lang/IllegalArgumentException" and untouched()
        stage(vm.env, self_, ins[0], ins[1], ins[2], h, w, vm.ints(flat), n, cells[0], cells[1], outs[0], vm.direct(out[1], out[1].nbytes - 1), outs[2])
        assert vm.take()[0] == "java/lang/IllegalArgumentException" and untouched()
        stage(vm.env, self_, ins[0], ins[1], ins[2], h, w, vm.ints(flat[:-1]), n, cells[0], cells[1], *outs)
        assert vm.take()[0] == "java/lang/IllegalArgumentException" and untouched()
        stage(vm.env, self_, ins[0], ins[1], ins[2], h, w, None, n, cells[0], cells[1], *outs)
        assert vm.take()[0] == "java/lang/IllegalArgumentException" and untouched()
        stage(vm.env, self_, ins[0], ins[1], ins[2], h, w, vm.ints(flat), -1, cells[0], cells[1], *outs)
        assert vm.take()[0] == "java/lang/IllegalArgumentException" and untouched()
        stage(vm.env, self_, ins[0], ins[1], ins[2], 0, w, vm.ints(flat), n, cells[0], cells[1], *outs)
        assert vm.take()[0] == "java/lang/IllegalArgumentException" and untouched()
        resident(vm.env, self_, vm.ints(flat[:4]), 2, cells[0], cells[1])
        assert vm.take()[0] == "java/lang/IllegalArgumentException"
        # the library's own refusals come through as the same class: a type above 26, a cell claimed twice, a block off the grid
        for bad in ([0, 0, 27], [0, 0, 0, 0, 0, 1], [2, 4, 4]):
            stage(vm.env, self_, ins[0], ins[1], ins[2], h, w, vm.ints(bad), len(bad) // 3, cells[0], cells[1], *outs)
            assert vm.take()[0] == "java/lang/IllegalArgumentException" and untouched()
            resident(vm.env, self_, vm.ints(bad), len(bad) // 3, cells[0], cells[1])
            assert vm.take()[0] == "java/lang/IllegalArgumentException"
        download(vm.env, self_, *[vm.direct(a) for a in down])
        assert vm.pending() is None and same(down)  # the refused calls left the resident planes as they were
        fresh = vm.fn("create", i64, i32)(vm.env, None, 0)
        resident(vm.env, vm.lib.fj_self(fresh), vm.ints(flat), n, cells[0], cells[1])
        assert vm.take()[0] == "java/lang/IllegalStateException"
        vm.fn("destroy", None, i64)(vm.env, None, fresh)
    finally:
        vm.fn("destroy", None, i64)(vm.env, None, handle)
