"""Contexts that launch on one main stream (jxl_ctx_set_stream) share one set of IDCT-output planes per frame size (host.hip,
PlanePool). Every case runs synthetic frames on such contexts and holds the outputs bit for bit to the same frames
run on contexts with streams of their own; the footprint query jxl_debug_intermediate_bytes tells whether a run took the pooled
set or private planes. A set is three f32 planes: 12 bytes per pixel.

The shared stream belongs to a `holder` context that runs nothing, so any of the others can be closed or moved first; the case
in which the stream's owner runs frames too (what bench.py does) has a test of its own.
"""
import ctypes as C
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, assert_bits_equal
from jxlatte_amd import _lib, abi, host, synth

pytestmark = pytest.mark.gpu


def _fitting_mix(w, h):
    """the default mix restricted to the types that fit a w x h frame"""
    return {n: s for n, s in synth.MIX_DEFAULT.items()
            if abi.TRANSFORM_TYPES[abi.TT_BY_NAME[n]][5] <= h and abi.TRANSFORM_TYPES[abi.TT_BY_NAME[n]][6] <= w}


def _subsampled():
    base = synth.make_vardct_frame(144, 80, seed=23, mix="dct8", xyb=0)
    return synth.make_subsampled(base, (1, 0, 1), (1, 0, 1))


# name -> (builder of the frame dict, stages or None)
CASES = {
    "A": (lambda: synth.make_vardct_frame(136, 72, seed=11, mix=_fitting_mix(136, 72)), None),
    "B": (lambda: synth.make_vardct_frame(72, 40, seed=12, mix=_fitting_mix(72, 40)), None),
    "C": (lambda: synth.make_vardct_frame(136, 72, seed=13, mix=_fitting_mix(136, 72)), None),
    "idct_only": (lambda: synth.make_vardct_frame(136, 72, seed=14, mix=_fitting_mix(136, 72)), abi.STAGE_IDCT),
    "epf3": (lambda: synth.make_vardct_frame(136, 72, seed=15, mix=_fitting_mix(136, 72), epf_iters=3), None),
    "sub": (_subsampled, None),
    "d8a": (lambda: synth.make_vardct_frame(136, 72, seed=17, mix="dct8"), None),
    "d8b": (lambda: synth.make_vardct_frame(136, 72, seed=18, mix="dct8"), None),
    "small": (lambda: synth.make_vardct_frame(136, 72, seed=19, mix={"DCT8": 0.4, "DCT4": 0.2, "HORNUSS": 0.1, "AFV0": 0.15, "DCT2": 0.15}), None),
    "wide": (lambda: synth.make_vardct_frame(128, 128, seed=16, mix={"DCT64_32": 0.45, "DCT32_64": 0.45}), None),
}
_frames, _expected = {}, {}


def _frame(name):
    if name not in _frames:
        _frames[name] = CASES[name][0]()
    return _frames[name]


def _reference(name):
    """the frame on a fresh context with a stream of its own, computed once"""
    if name not in _expected:
        with _lib.Context(0) as c:
            _expected[name] = host.Frame.from_synth(c, _frame(name), stages=CASES[name][1]).decodeFrame().copy()
    return _expected[name]


def _set_bytes(name):
    return 12 * _frame(name)["width"] * _frame(name)["height"]


def _inter_bytes():
    f = _lib.load().jxl_debug_intermediate_bytes
    f.restype, f.argtypes = C.c_int64, [C.c_int]
    return f(0)


class _Shared:
    """a holder context (it only lends its stream) and n contexts on that stream; `grew()`: intermediate bytes allocated since"""

    def __init__(self, n):
        self.before = _inter_bytes()
        self.holder = _lib.Context(0)
        self.ctxs = [_lib.Context(0) for _ in range(n)]
        for c in self.ctxs:
            c.call("jxl_ctx_set_stream", self.holder.stream)

    def grew(self):
        return _inter_bytes() - self.before

    def close(self):
        for c in self.ctxs:
            c.close()
        self.holder.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def _load(ctx, name):
    return host.Frame.from_synth(ctx, _frame(name), stages=CASES[name][1])


def test_three_contexts_share_one_set_per_size_and_results_outlive_siblings():
    exp = {n: _reference(n) for n in "ABC"}
    with _Shared(3) as sh:
        fa, fb, fc = (_load(c, n) for c, n in zip(sh.ctxs, "ABC"))
        assert sh.grew() == 0  # nothing is allocated before a run needs it
        fa.run()
        fb.run()
        fc.run()
        oc, oa, ob = fc.readOutput(), fa.readOutput(), fb.readOutput()  # A after C has run: results never live in the pool
        assert_bits_equal(oc, exp["C"], "C")
        assert_bits_equal(oa, exp["A"], "A, read after B and C ran")
        assert_bits_equal(ob, exp["B"], "B")
        assert sh.grew() == _set_bytes("A") + _set_bytes("B")  # one set per size class, not three
    assert _inter_bytes() == sh.before  # the last context out frees the sets


def test_repeated_interleaving_without_host_synchronisation():
    exp = {n: _reference(n) for n in "ABC"}
    with _Shared(3) as sh:
        fr = dict(zip("ABC", (_load(c, n) for c, n in zip(sh.ctxs, "ABC"))))
        for _ in range(5):
            for n in "ABACB":
                fr[n].run()
        for n in "ABC":
            assert_bits_equal(fr[n].readOutput(), exp[n], n)
        assert sh.grew() == _set_bytes("A") + _set_bytes("B")


def test_the_streams_owner_joins_the_pool():
    """bench.py's order: the owner of the stream opens its frame (private planes, it is alone), then others are put on its
    stream: from its next run on the owner uses the pooled set and its private planes are gone"""
    exp = {n: _reference(n) for n in "AC"}
    before = _inter_bytes()
    c1, c2 = _lib.Context(0), _lib.Context(0)
    try:
        f1 = _load(c1, "A")
        assert _inter_bytes() - before == _set_bytes("A")
        f1.run()
        c2.call("jxl_ctx_set_stream", c1.stream)
        f2 = _load(c2, "C")
        for _ in range(3):
            f1.run()
            f2.run()
        o2, o1 = f2.readOutput(), f1.readOutput()
        assert_bits_equal(o1, exp["A"], "owner")
        assert_bits_equal(o2, exp["C"], "guest")
        assert _inter_bytes() - before == _set_bytes("A")  # one pooled set, no private one
    finally:
        c2.close()
        c1.close()
    assert _inter_bytes() == before


@pytest.mark.parametrize("name", ["idct_only", "epf3", "sub"])
def test_runs_whose_intermediate_outlives_them_take_private_planes(name):
    """stage-masked (the result IS the IDCT output), the EPF x 3 pair with f32 out, a chroma-subsampled frame: each with a
    sibling's run behind it on the stream, and read last"""
    exp, exp_c = _reference(name), _reference("C")
    with _Shared(2) as sh:
        f1, f2 = _load(sh.ctxs[0], name), _load(sh.ctxs[1], "C")
        for _ in range(2):
            f1.run()
            f2.run()
        o2, o1 = f2.readOutput(), f1.readOutput()
        assert_bits_equal(o2, exp_c, "sibling")
        assert_bits_equal(o1, exp, name)
        assert sh.grew() == _set_bytes(name) + _set_bytes("C")  # private planes of the first + the sibling's pooled set


def test_copy_output_device_reads_the_result_not_the_pool():
    """jxl_vardct_copy_output_device after a sibling has run: it reads result[], which is never a pooled plane, so the run
    itself stays pooled"""
    lib = _lib.load()
    exp = _reference("A")
    with _Shared(2) as sh:
        f1, f2 = _load(sh.ctxs[0], "A"), _load(sh.ctxs[1], "C")
        f1.run()
        f2.run()
        dev, got = C.c_void_p(), np.empty_like(exp)
        assert lib.hipMalloc(C.byref(dev), C.c_size_t(exp.nbytes)) == 0
        try:
            sh.ctxs[0].call("jxl_vardct_copy_output_device", dev)
            sh.ctxs[0].synchronize()
            assert lib.hipMemcpy(C.c_void_p(got.ctypes.data), dev, C.c_size_t(exp.nbytes), 2) == 0  # hipMemcpyDeviceToHost
        finally:
            lib.hipFree(dev)
        assert_bits_equal(got, exp, "device copy")
        assert_bits_equal(f2.readOutput(), _reference("C"), "sibling")
        assert sh.grew() == _set_bytes("A")


@pytest.mark.parametrize("pair", [("A", "C"), ("d8a", "d8b")])
def test_run_batch_keeps_private_planes(pair):
    """host.Frame.runBatch over two 136 x 72 frames of the stream: the default mix (larger varblocks: the call falls back to plain
    runs) and all-DCT8 frames (the shared IDCT launches); a third context holds the 72 x 40 frame"""
    exp = {"A": _reference(pair[0]), "C": _reference(pair[1]), "B": _reference("B")}
    with _Shared(3) as sh:
        fa, fb, fc = (_load(c, n) for c, n in zip(sh.ctxs, pair + ("B",)))
        fa.run()
        fb.run()
        host.Frame.runBatch([fa, fb])
        fc.run()
        fa.run()  # and back to the pooled set
        ob, oc, oa = fb.readOutput(), fc.readOutput(), fa.readOutput()
        assert_bits_equal(oa, exp["A"], "A")
        assert_bits_equal(ob, exp["C"], "C")
        assert_bits_equal(oc, exp["B"], "B")
        # pooled: one 136 x 72 set and one 72 x 40 set; private: the two batched contexts
        assert sh.grew() == 3 * _set_bytes("A") + _set_bytes("B")


def test_run_batch_sees_a_new_frame_on_one_context_of_the_batch():
    """two guests of the stream that have run nothing: the batch allocates their private planes itself, which invalidates the cached
    argument blocks of the batch; then a new frame with another block layout on the second context only, and the batch again. The
    keys of that cache must be unique per (context, tables): the second batch must not replay the first one's blocks"""
    exp = {n: _reference(n) for n in ("d8a", "d8b", "small")}
    assert len(_frame("small")["block_types"]) != len(_frame("d8b")["block_types"]) or \
        not np.array_equal(_frame("small")["block_types"], _frame("d8b")["block_types"])
    with _Shared(2) as sh:
        fx, fy = _load(sh.ctxs[0], "d8a"), _load(sh.ctxs[1], "d8b")
        host.Frame.runBatch([fx, fy])
        oy, ox = fy.readOutput(), fx.readOutput()
        assert_bits_equal(ox, exp["d8a"], "first batch, first context")
        assert_bits_equal(oy, exp["d8b"], "first batch, second context")
        fy = _load(sh.ctxs[1], "small")
        host.Frame.runBatch([fx, fy])
        oy, ox = fy.readOutput(), fx.readOutput()
        assert_bits_equal(ox, exp["d8a"], "second batch, first context")
        assert_bits_equal(oy, exp["small"], "second batch, the new frame")
        assert sh.grew() == 2 * _set_bytes("d8a")


def test_a_frame_without_the_idct_stage_starts_from_zero_planes_everywhere():
    """the stage mask belongs to begin_frame, and begin_frame starts a frame from zeroed output planes unless the IDCT stage of
    a fully tiled frame overwrites them: a frame opened with the IDCT bit clear never sees an earlier run's IDCT output, on a
    private stream or behind a pooled run, and gives the same planes in both places"""
    rest = abi.STAGE_ALL & ~abi.STAGE_IDCT
    with _lib.Context(0) as c:
        host.Frame.from_synth(c, _frame("A")).run()
        alone = host.Frame.from_synth(c, _frame("A"), stages=rest).decodeFrame().copy()
    assert not np.array_equal(alone, _reference("A"))  # it did not restore the previous run's IDCT output
    assert all(len(np.unique(alone[ch].view(np.uint32))) == 1 for ch in range(3))  # ... but constant planes: those of zeros
    with _Shared(2) as sh:
        _load(sh.ctxs[0], "A").run()
        _load(sh.ctxs[1], "C").run()
        got = host.Frame.from_synth(sh.ctxs[0], _frame("A"), stages=rest).decodeFrame()
        assert_bits_equal(got, alone, "behind a pooled run")
        assert_bits_equal(_load(sh.ctxs[0], "A").decodeFrame(), _reference("A"), "and whole frames as before")


def test_side_stream_launch_directly_behind_a_siblings_run():
    """DCT64_32 / DCT32_64 blocks are the 512-thread class, launched on the context's side stream: ten times back to back behind
    a sibling's run on the shared stream"""
    exp, exp_c = _reference("wide"), _reference("A")
    with _Shared(2) as sh:
        fw, fs = _load(sh.ctxs[0], "wide"), _load(sh.ctxs[1], "A")
        types = set(abi.TRANSFORM_TYPES[t][0] for t in _frame("wide")["block_types"])
        assert {"DCT64_32", "DCT32_64", "DCT8"} <= types  # both IDCT classes: the 512-thread one goes to the side stream
        for _ in range(10):
            fs.run()
            fw.run()
        assert_bits_equal(fw.readOutput(), exp, "wide blocks")
        fs.run()
        fw.run()
        fs.run()
        os_, ow = fs.readOutput(), fw.readOutput()
        assert_bits_equal(os_, exp_c, "sibling")
        assert_bits_equal(ow, exp, "wide blocks, read after the sibling")
        assert sh.grew() == _set_bytes("wide") + _set_bytes("A")


def test_reattachment():
    exp = _reference("A")
    with _Shared(2) as sh, _lib.Context(0) as other:
        c = sh.ctxs[0]
        f, fs = _load(c, "A"), _load(sh.ctxs[1], "C")
        f.run()
        fs.run()
        first = f.readOutput()
        c.call("jxl_ctx_set_stream", other.stream)  # a stream nothing else launches on
        fs.run()
        f.run()
        second = f.readOutput()
        assert_bits_equal(first, exp, "on the shared stream")
        assert_bits_equal(second, exp, "on its own stream")
        assert_bits_equal(fs.readOutput(), _reference("C"), "the context left behind")
        assert sh.grew() == 2 * _set_bytes("A")  # one set on either stream


def test_close_while_a_siblings_runs_are_queued():
    exp = _reference("C")
    with _Shared(2) as sh:
        f1, f2 = _load(sh.ctxs[0], "A"), _load(sh.ctxs[1], "C")
        for _ in range(8):
            f1.run()
            f2.run()
        sh.ctxs[0].close()
        f2.run()
        assert_bits_equal(f2.readOutput(), exp, "sibling of a closed context")
        assert _lib.load().hipDeviceSynchronize() == 0
        assert sh.grew() == _set_bytes("C")


_CHILD = r"""
import hashlib, sys, ctypes as C
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import test_shared_planes_gpu as t
from jxlatte_amd import _lib
with t._Shared(3) as sh:
    fr = [t._load(c, n) for c, n in zip(sh.ctxs, "ABC")]
    for f in fr:
        f.run()
    outs = [fr[i].readOutput() for i in (2, 0, 1)]
    print("RESULT", sh.grew(), *[hashlib.sha256(o.tobytes()).hexdigest() for o in outs])
"""


def test_switch_off_gives_every_context_its_own_planes():
    exp = [hashlib.sha256(np.ascontiguousarray(_reference(n)).tobytes()).hexdigest() for n in "CAB"]
    env = dict(os.environ, JXL_SHARED_PLANES="0")
    r = subprocess.run([sys.executable, "-c", _CHILD % (ROOT, os.path.join(ROOT, "tests"))], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT")][-1].split()
    assert int(line[1]) == 2 * _set_bytes("A") + _set_bytes("B")  # one set per context
    assert line[2:] == exp
