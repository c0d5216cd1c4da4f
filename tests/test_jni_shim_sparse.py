"""The sparse-feed natives of integration/jni/jxlatte_amd_jni.c (putGroupSparse, mapSparse, commitSparse, sparseRejected), called
through ctypes over tests/stubs/fake_jni.c as tests/test_jni_shim.py calls the dense ones: a frame fed through them equals the same
frame through the C-ABI, and their argument checks arrive as the Java exception classes."""
import ctypes as C

import numpy as np
import pytest

from test_jni_shim import FakeJVM, _build


def _begin(vm, self_, frame, params):
    i32, vp = C.c_int32, C.c_void_p
    pbuf = np.frombuffer(bytes(params), np.uint8).copy()
    vm.fn("beginFrame", None, vp)(vm.env, self_, vm.direct(pbuf))
    assert vm.pending() is None, vm.pending()
    w = np.ascontiguousarray(frame["weights"], np.float32)
    vm.fn("setWeights", None, vp, vp)(vm.env, self_, vm.direct(w), vm.ints(frame["woffs"]))
    assert vm.pending() is None, vm.pending()
    set_lfg = vm.fn("setLFGroup", None, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp)
    for g in frame["lfgroups"]:
        a = {k: np.ascontiguousarray(g[k]) for k in ("dct_select", "hf_mul", "sharpness", "x_from_y", "b_from_y", "block_yx")}
        lf = [np.ascontiguousarray(p, np.float32) for p in g["lf"]]
        ch, cw = a["dct_select"].shape
        set_lfg(vm.env, self_, int(g["lfg_y"]), int(g["lfg_x"]), ch, cw, vm.direct(a["dct_select"].astype(np.uint8)),
                vm.direct(a["hf_mul"].astype(np.int32)), vm.direct(a["sharpness"].astype(np.int32)), vm.direct(a["x_from_y"].astype(np.int32)),
                vm.direct(a["b_from_y"].astype(np.int32)), vm.direct(a["block_yx"].astype(np.int32)), a["block_yx"].shape[0],
                vm.direct(lf[0]), vm.direct(lf[1]), vm.direct(lf[2]))
        assert vm.pending() is None, vm.pending()


@pytest.mark.gpu
def test_frame_through_the_sparse_jni_entries_equals_the_c_abi(ctx, tmp_path):
    from conftest import assert_bits_equal
    from jxlatte_amd import abi, host, synth
    from jxlatte_amd.host import pack_sparse
    vm = FakeJVM(_build(tmp_path))
    i32, i64, vp = C.c_int32, C.c_int64, C.c_void_p
    frame = synth.make_vardct_frame(320, 200, seed=41, mix="all")
    frame["coeff"][1, 9, 3] = 70000  # one value for the wide form
    exp = host.Frame.from_synth(ctx, frame).decodeFrame()
    H, W = exp.shape[1:]
    n_groups = synth.num_groups(frame)

    handle = vm.fn("create", i64, i32)(vm.env, None, 0)
    assert handle and vm.pending() is None
    self_ = vm.lib.fj_self(handle)
    run = vm.fn("run", None)
    read = vm.fn("readOutput", None, vp, vp, vp, i64)
    put = vm.fn("putGroupSparse", None, i32, i32, vp, vp, vp, i32, i32, i32, C.c_uint8)
    map_ = vm.fn("mapSparse", vp, i64)
    commit = vm.fn("commitSparse", None, vp)
    rejected = vm.fn("sparseRejected", i64)

    def result():
        run(vm.env, self_)
        assert vm.pending() is None, vm.pending()
        out = [np.zeros((H, W), np.float32) for _ in range(3)]
        read(vm.env, self_, vm.direct(out[0]), vm.direct(out[1]), vm.direct(out[2]), W)
        assert vm.pending() is None, vm.pending()
        return np.stack(out)

    try:
        params = abi.VarDCTParams.from_buffer_copy(frame["params"])
        # putGroupSparse, group by group (a group with a value outside int16 in the wide form)
        _begin(vm, self_, frame, params)
        for grp in range(n_groups):
            q = synth.group_view(frame, grp)
            wide = any(int(np.abs(a).max()) > 32767 for a in q)
            e = [pack_sparse(a, wide) for a in q]
            put(vm.env, self_, 0, grp, vm.direct(e[0]), vm.direct(e[1]), vm.direct(e[2]), *[a.size // (2 if wide else 1) for a in e], wide)
            assert vm.pending() is None, vm.pending()
        assert_bits_equal(result(), exp, "putGroupSparse over JNI vs C-ABI")
        assert rejected(vm.env, self_) == 0 and vm.pending() is None

        # mapSparse + commitSparse: the buffer comes back as ONE direct buffer of exactly the asked size
        _begin(vm, self_, frame, params)
        cap = (2 * int(np.count_nonzero(frame["coeff"])) + 12 * n_groups + 16) & ~3
        buf = map_(vm.env, self_, cap)
        assert vm.pending() is None and buf, vm.pending()
        assert vm.lib.fj_length(buf) == 4 * cap
        words = np.ctypeslib.as_array(C.cast(vm.lib.fj_data(buf), C.POINTER(C.c_uint32)), shape=(cap,))
        runs, at = [], 0
        for grp in range(n_groups):
            for c, a in enumerate(synth.group_view(frame, grp)):
                wide = int(np.abs(a).max()) > 32767
                e = pack_sparse(a, wide)
                words[at:at + e.size] = e
                runs += [grp, c, 1 if wide else 0, e.size // (2 if wide else 1), at]
                at += (e.size + 3) & ~3
        commit(vm.env, self_, vm.ints(runs))
        assert vm.pending() is None, vm.pending()
        assert_bits_equal(result(), exp, "commitSparse over JNI vs C-ABI")

        # argument checks: a buffer shorter than its count, a run list that is not five ints per run, a run the library refuses,
        # a commit before mapSparse
        e = pack_sparse(synth.group_view(frame, 0)[0])
        put(vm.env, self_, 0, 0, vm.direct(e, e.nbytes - 4), None, None, e.size, 0, 0, False)
        assert vm.take()[0] == "java/lang/IllegalArgumentException"
        put(vm.env, self_, 0, n_groups, vm.direct(e), None, None, e.size, 0, 0, False)
        assert vm.take()[0] == "java/lang/IllegalArgumentException"
        commit(vm.env, self_, vm.ints([0, 0, 0, 1]))
        assert vm.take()[0] == "java/lang/IllegalArgumentException"
        commit(vm.env, self_, vm.ints([0, 3, 0, 1, 0]))
        assert vm.take()[0] == "java/lang/IllegalArgumentException"
        map_(vm.env, self_, 0)
        assert vm.take()[0] == "java/lang/IllegalArgumentException"
        _begin(vm, self_, frame, params)
        commit(vm.env, self_, vm.ints([0, 0, 0, 1, 0]))
        assert vm.take()[0] == "java/lang/IllegalStateException"
    finally:
        vm.fn("destroy", None, i64)(vm.env, None, handle)
