"""The native of integration/jni/jxlatte_amd_jni.c that jxl_modular_begin_chain adds (modularBeginChain), called through ctypes
over tests/stubs/fake_jni.c as tests/test_jni_shim_frames.py calls the others: the plan it makes gives the model's channels, and its
own size checks and the library's refusals arrive as the Java exception classes."""
import ctypes as C

import numpy as np
import pytest

import modchain_cases as cases
from test_jni_shim import FakeJVM, _build


def _flat(transforms):
    tr = [v for t in transforms for v in (t["kind"], t["begin_c"], t["num_c"], t["rct_type"], t["nb_colors"], t["nb_deltas"], t["d_pred"], len(t["steps"]))]
    return tr, [v for t in transforms for s in t["steps"] for v in s]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["sample_shape_5x7", "palette_squeeze"])
def test_chain_entry_over_jni_gives_the_models_channels(tmp_path, name):
    vm = FakeJVM(_build(tmp_path))
    i32, i64, vp = C.c_int32, C.c_int64, C.c_void_p
    vm.lib.fj_objects.restype, vm.lib.fj_objects.argtypes = vp, [i64]
    vm.lib.fj_set_object.restype, vm.lib.fj_set_object.argtypes = None, [vp, i64, vp]
    c = cases.CASES[name]
    chans = [np.ascontiguousarray(a) for a in c["chans"]]
    tr, steps = _flat(c["transforms"])
    handle = vm.fn("create", i64, i32)(vm.env, None, 0)
    assert handle and vm.pending() is None
    self_ = vm.lib.fj_self(handle)
    begin = vm.fn("modularBeginChain", None, vp, vp, vp, vp, vp, i32)

    def objects(arrays, sizes=None):
        arr = vm.lib.fj_objects(len(arrays))
        for k, a in enumerate(arrays):
            vm.lib.fj_set_object(arr, k, vm.direct(a, None if sizes is None else sizes[k]))
        return arr
    widths, heights = [a.shape[1] for a in chans], [a.shape[0] for a in chans]
    try:
        begin(vm.env, self_, objects(chans), vm.ints(widths), vm.ints(heights), vm.ints(tr), vm.ints(steps), c["bit_depth"])
        assert vm.pending() is None, vm.pending()
        vm.fn("modularRun", None)(vm.env, self_)
        assert vm.pending() is None, vm.pending()
        want = cases.expected(name)
        assert vm.fn("modularOutCount", i32)(vm.env, self_) == len(want)
        for k, w in enumerate(want):
            got = np.full(w.shape, -77, np.int32)
            vm.fn("modularReadChannel", None, i32, vp)(vm.env, self_, k, vm.direct(got))
            assert vm.pending() is None, vm.pending()
            assert np.array_equal(got, w), (name, k)

        def refused(cls, **change):
            a = dict(chans=objects(chans), widths=vm.ints(widths), heights=vm.ints(heights), tr=vm.ints(tr), steps=vm.ints(steps), depth=c["bit_depth"])
            a.update(change)
            begin(vm.env, self_, a["chans"], a["widths"], a["heights"], a["tr"], a["steps"], a["depth"])
            got = vm.take()
            assert got is not None and got[0] == cls, (change, got)
        arg = "java/lang/IllegalArgumentException"
        refused(arg, chans=objects(chans, [a.nbytes for a in chans[:-1]] + [chans[-1].nbytes - 4]))  # a short channel
        refused(arg, widths=vm.ints(widths[:-1]))                                                    # a short size array
        refused(arg, tr=vm.ints(tr[:-8] + tr[-8:-1] + [tr[-1] + 1]))                                # more steps counted than given
        refused(arg, depth=0)                                                                        # the library's own
        bad = list(tr)
        bad[0] = 3
        refused(arg, tr=vm.ints(bad))
        if name == "sample_shape_5x7":
            weighted = list(tr)
            weighted[5], weighted[6] = 1, 6  # nb_deltas 1, d_pred 6 on the Palette undone last
            refused("java/lang/UnsupportedOperationException", tr=vm.ints(weighted))
        # nothing was queued by the refused calls: the plan made first is still the context's
        assert vm.fn("modularOutCount", i32)(vm.env, self_) == len(want)
    finally:
        vm.fn("destroy", None, i64)(vm.env, None, handle)
