"""The run-time switches of the library (every getenv("JXL_...") under jxlatte_amd/csrc/) and the cases that force them.

Two lists, kept complete by tests/test_switch_inventory_cpu.py: RESULT_PATH -- switches that select other device code or another
launch plan, each with the test that forces it -- and DIAGNOSTIC_ONLY. The second half of the module is the body of the child
processes of tests/test_switches_gpu.py: a switch the library reads once per process can only be forced in a fresh process, so

    JXL_RESTORE_PH=2 python tests/switch_cases.py restore_ph2

decodes that case's frames with the switch set, compares each with the oracle bit for bit, prints one line per comparison and
"RESULT <failed comparisons>", and exits non-zero if any failed. The same command under a kernel trace shows which kernels the
switch selected. Importing the module needs neither the device library nor a GPU."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))

_SW = "test_switches_gpu.py::"
# switch -> the test that forces it (file under tests/ :: test function)
RESULT_PATH = {
    "JXL_RESTORE_PH": _SW + "test_restore_4x2_patches",
    "JXL_RESTORE_LDS_PAD": _SW + "test_restore_lds_pad",
    "JXL_AUX_STREAMS": _SW + "test_aux_streams",
    "JXL_NO_BATCH": _SW + "test_no_batch",
    "JXL_NO_BATCH_RESTORE": _SW + "test_no_batch_restore",
    "JXL_PQ_F64": _SW + "test_f64_transfer_forms_per_context",
    "JXL_SRGB8_F64": _SW + "test_f64_transfer_forms_per_context",
    "JXL_PQ16_F64": _SW + "test_f64_transfer_forms_16_bit",
    "JXL_SRGB16_F64": _SW + "test_f64_transfer_forms_16_bit",
    "JXL_COMMIT_ZEROCOPY": _SW + "test_bus_paths",
    "JXL_TABLE_ZEROCOPY": _SW + "test_bus_paths",
    "JXL_OUTPUT_ZEROCOPY": _SW + "test_bus_paths",
    "JXL_WIDEN_GRID": _SW + "test_bus_paths",
    "JXL_OUTPUT_GRID": _SW + "test_bus_paths",
    "JXL_SQUEEZE_NO_CHAIN": _SW + "test_squeeze_no_chain",
    "JXL_SQUEEZE_CHAIN_MAX": _SW + "test_squeeze_chain_max",
    "JXL_SQUEEZE_SHORT_MAX": _SW + "test_squeeze_short_max",
    "JXL_SQUEEZE_NO_TAIL": _SW + "test_squeeze_no_tail",
    "JXL_SQUEEZE_SERIAL": _SW + "test_squeeze_serial_small",
    "JXL_VH_TILES": _SW + "test_vh_geometry",
    "JXL_VH_SMALL": _SW + "test_vh_geometry",
    "JXL_VH_CW32_MINSEG": _SW + "test_vh_geometry",
    # forced by tests that were there before test_switches_gpu.py (which lists them in PINNED_ELSEWHERE)
    "JXL_EPF3_SPLIT": "test_experimental_kernels_gpu.py::test_three_epf_iterations_as_one_launch_and_as_two",
    "JXL_WG3_GRID": "test_experimental_kernels_gpu.py::test_switched_kernel_is_bit_exact",
    "JXL_WG3_GRID_BIG": "test_experimental_kernels_gpu.py::test_switched_kernel_is_bit_exact",
    "JXL_SHARED_PLANES": "test_shared_planes_gpu.py::test_switch_off_gives_every_context_its_own_planes",
    "JXL_HSQUEEZE_WALK_MAX": "test_modular_gpu.py::test_segmented_squeeze_random",
    "JXL_SQUEEZE_SPECULATE": "test_modular_gpu.py::test_plan_with_speculative_checks_redoes_adversarial_rows",
    "JXL_SQUEEZE_NO_VH": "test_modular_gpu.py::test_fused_plan_equals_unfused_plan",
    "JXL_VH_SEG": "test_modular_gpu.py::test_fused_vh_pair",
    "JXL_VH_CW": "test_modular_gpu.py::test_fused_vh_pair",
}

# switch -> why no parity test is owed
DIAGNOSTIC_ONLY = {
    "JXL_PREPARE_TIMING": "prints host timings of jxl_vardct_prepare's sections to stderr; selects no device code and no launch",
    "JXL_VH_ABL": "read only in a library built with -DJXL_VH_ABL (ablations of k_modular_vh.hip); the shipped build has no such getenv",
}

# ---- shared between the parent tests and the children -------------------------------------------------------------------------
# frame edges on both sides of the 64-wide, 32-row window and of the 62x30 / 58x26 output tiles. (64, 32) is ONE window exactly
# (the frame edge on the tile edge of EPF iterations 0 / 1) and leaves a remnant of one 4x2 patch row and half a patch column to the
# 62x30 tiles of two iterations. A patch row that straddles the frame's bottom edge inside the LAST stage cannot occur: frame heights
# are multiples of 8, tile origins multiples of 32 / 30 / 26, so the last stage's patch rows start on even frame rows; the stages
# before it start one row off (halo 1 or 3), so their patches straddle the bottom edge at every size here.
RESTORE_SIZES = ((72, 40), (136, 72), (520, 264), (264, 1000), (64, 32))
# extra dynamic LDS of the JXL_RESTORE_LDS_PAD test: 35 188 bytes of the kernel's own (Geo<GAB, 1 or 2>::LDS_BYTES) + 16 KiB = 51 572,
# 66 724 + 16 KiB = 83 108 for the 64x64 window of a split three-iteration frame: under the 160 KiB a workgroup may ask for, and
# it moves the workgroups per CU (4 -> 3)
LDS_PAD_BYTES = 16384
AUX_MAX = 12  # jxl_ctx::kAux (host.hip)


def batch_frames(kind):
    """the two batches of the JXL_NO_BATCH / JXL_NO_BATCH_RESTORE tests: "mixed" = four frames whose restoration variants differ
    (Gaborish on / off, 0 / 1 / 2 EPF iterations), "one" = four frames of one variant at different sizes"""
    from jxlatte_amd import synth
    if kind == "mixed":
        spec = [((136, 72), True, 2), ((136, 72), False, 2), ((72, 40), True, 1), ((136, 72), True, 0)]
    else:
        spec = [((136, 72), True, 2), ((264, 136), True, 2), ((136, 72), True, 2), ((72, 40), True, 2)]
    return [synth.make_vardct_frame(s[0], s[1], seed=300 + 10 * (kind == "one") + i, mix="default", aligned=False, epf_iters=it, gab=g)
            for i, (s, g, it) in enumerate(spec)]


def transfer_inputs():
    """the inputs of test_transfer_pq_exact_form (tests/test_stages_gpu.py) plus the sRGB knee"""
    import numpy as np
    rng = np.random.default_rng(99)
    return np.concatenate([rng.random(200000), rng.random(20000) * 1e-3, rng.random(20000) * 4.0,
                           [0.0, 1.0, 0.5, 0.0031306, 0.0031307]]).astype(np.float32)


def sink_frames():
    """(frame, transfer, format name) of the frame-sink transfer cases: stage set 31, PQ and sRGB, the four integer formats"""
    from jxlatte_amd import abi, synth
    out = []
    for size, seed in (((96, 64), 41), ((72, 40), 42)):
        base = synth.make_vardct_frame(size[0], size[1], seed=seed, mix="default", aligned=False)
        for tf in (abi.TRANSFER_PQ, abi.TRANSFER_SRGB):
            for fmt in ("U8", "U16", "RGB8", "RGB16"):
                out.append((with_params(base, 31, transfer=tf, out_format=getattr(abi, "OUT_" + fmt)), tf, fmt))
    return out


def with_params(frame, stages, **fields):
    """a copy of a synth frame with other header fields (the coefficient data does not depend on them)"""
    from jxlatte_amd import abi
    p = abi.VarDCTParams.from_buffer_copy(frame["params"])
    p.stages = stages
    for k, v in fields.items():
        setattr(p, k, v)
    f2 = dict(frame)
    f2["params"] = p
    return f2


def planar(got):
    """the device result in the oracle's layout: [3][H][W], int32 for the integer formats"""
    import numpy as np
    got = np.asarray(got)
    if got.dtype == np.float32:
        return got
    if got.ndim == 3 and got.shape[-1] == 3 and got.shape[0] != 3:
        got = np.moveaxis(got, -1, 0)
    return np.ascontiguousarray(got, np.int32)


def bus_frames():
    """frames of the bus-path cases: float planes, an interleaved 8-bit and a planar 16-bit sink; one 4:2:0 frame, whose mapped planes
    differ in size. (Its subsampled planes are 24 rows high. A subsampled plane whose height is no multiple of 8 -- the staged
    fall-back of commit_i16 -- cannot be made here: synth.make_subsampled takes frames of whole 16x16 cells only.)"""
    from jxlatte_amd import abi, synth
    a = synth.make_vardct_frame(264, 136, seed=61, mix="default", aligned=False)
    b = synth.make_vardct_frame(1000, 520, seed=62, mix="default", aligned=False)
    sub = synth.make_subsampled(synth.make_vardct_frame(80, 48, seed=63, mix="dct8", xyb=0), (1, 0, 1), (1, 0, 1))
    return [("264x136 f32", with_params(a, 15)),
            ("264x136 rgb8", with_params(a, 31, transfer=abi.TRANSFER_SRGB, out_format=abi.OUT_RGB8)),
            ("1000x520 f32", with_params(b, 15)),
            ("1000x520 u16", with_params(b, 31, transfer=abi.TRANSFER_SRGB, out_format=abi.OUT_U16)),
            ("80x48 4:2:0 f32", with_params(sub, 7))]


# ---- the children ---------------------------------------------------------------------------------------------------------------
class _Tally:
    def __init__(self):
        self.bad = 0

    def check(self, got, exp, what):
        from conftest import assert_bits_equal
        try:
            assert_bits_equal(got, exp, what)
            print("ok  ", what, flush=True)
        except AssertionError as e:
            self.bad += 1
            print("FAIL", e, flush=True)


def _restore(sizes, its, batch_iters):
    from jxlatte_amd import _lib, host, synth
    from oracle import pyoracle as orc
    t = _Tally()
    ctx = _lib.Context(0)
    for i, size in enumerate(sizes):
        base = synth.make_vardct_frame(size[0], size[1], seed=70 + i, mix="default", aligned=False)
        for it in its:
            for gab in (1, 0):
                for st in (7, 15):  # float planes out: the plain sink, the only one with 4x2 instantiations
                    f = with_params(base, st, epf_iters=it, gab=gab)
                    fr = host.Frame.from_synth(ctx, f, stages=st)
                    t.check(fr.decodeFrame(), orc.vardct_frame(f, stages=st),
                            "%dx%d epf %d gab %d stages %d (%d launches)" % (size[0], size[1], it, gab, st, fr.lastLaunchCount()))
    ctx.close()
    ctxs = [_lib.Context(0) for _ in range(3)]
    frames = [synth.make_vardct_frame(264, 136, seed=20 + i, mix="default", epf_iters=batch_iters) for i in range(3)]
    frs = [host.Frame.from_synth(c, f, stages=15) for c, f in zip(ctxs, frames)]
    host.Frame.runBatch(frs)
    for i, (fr, f) in enumerate(zip(frs, frames)):
        t.check(fr.readOutput(), orc.vardct_frame(f, stages=15), "batch frame %d epf %d" % (i, batch_iters))
    for c in ctxs:
        c.close()
    return t.bad


def case_restore_ph2():
    return _restore(RESTORE_SIZES, (0, 1, 2, 3), 2)


def case_restore_ph2_epf3():
    return _restore(RESTORE_SIZES, (3,), 3)


def case_restore_lds_pad():
    return _restore(((136, 72), (520, 264)), (1, 2), 2)


def case_no_batch_restore():
    """both batches against the oracle; prints the one-variant batch's summed launch count for the parent to place"""
    from jxlatte_amd import _lib, host
    from oracle import pyoracle as orc
    t = _Tally()
    for kind in ("mixed", "one"):
        frames = batch_frames(kind)
        ctxs = [_lib.Context(0) for _ in frames]
        frs = [host.Frame.from_synth(c, f, stages=15) for c, f in zip(ctxs, frames)]
        host.Frame.runBatch(frs)
        for i, (fr, f) in enumerate(zip(frs, frames)):
            t.check(fr.readOutput(), orc.vardct_frame(f, stages=15), "%s batch frame %d" % (kind, i))
        print("COUNT", kind, sum(fr.lastLaunchCount() for fr in frs), flush=True)
        for c in ctxs:
            c.close()
    return t.bad


def case_transfer16():
    """JXL_PQ16_F64 / JXL_SRGB16_F64: 16-bit code values through jxl_stage_transfer and through the frame sink; prints the largest
    difference and the differing share per comparison for the parent to hold against the project's bar"""
    import numpy as np
    from jxlatte_amd import _lib, abi, host
    from oracle import pyoracle as orc
    ctx = _lib.Context(0)
    x = transfer_inputs()
    for name, tf in (("PQ", abi.TRANSFER_PQ), ("SRGB", abi.TRANSFER_SRGB)):
        d = np.abs(host.transfer(ctx, x, tf, 65535).astype(np.int64) - orc.transfer(x, tf, 65535))
        print("DIFF stage %s max %d share %.3e" % (name, int(d.max()), float((d != 0).mean())), flush=True)
    for f, tf, fmt in sink_frames():
        if fmt in ("U16", "RGB16"):
            got = planar(host.Frame.from_synth(ctx, f).decodeFrame())
            d = np.abs(got.astype(np.int64) - orc.vardct_frame(f))
            print("DIFF sink %s %s %dx%d max %d share %.3e" % ("PQ" if tf == abi.TRANSFER_PQ else "SRGB", fmt, f["width"], f["height"],
                                                              int(d.max()), float((d != 0).mean())), flush=True)
    ctx.close()
    return 0


def _bus_one(t, ctx, lib, name, f):
    """one frame through the mapped int16 planes and a page-locked destination (both read_output forms), against the oracle and
    against putGroup + a pageable read"""
    import ctypes as C
    import numpy as np
    from jxlatte_amd import abi, host, synth
    from oracle import pyoracle as orc
    p = abi.VarDCTParams.from_buffer_copy(f["params"])
    exp = orc.vardct_frame(f)
    plain = host.Frame.from_synth(ctx, f).decodeFrame()  # putGroup, pageable destination
    t.check(planar(plain), exp, name + ": putGroup + pageable read")
    fr = host.Frame(ctx, p, f["weights"], f["woffs"])
    for g in f["lfgroups"]:
        fr.setLFGroup(g)
    planes = fr.mapCoeffsI16()
    src, _, _ = synth.channel_planes(f)
    for c in range(3):
        planes[c][...] = src[c]
    fr.commitCoeffsI16()
    fr.run()
    pin = host.PinnedArray(lib, plain.shape, plain.dtype)
    try:
        il = plain.ndim == 3 and plain.shape[-1] == 3 and plain.dtype != np.float32
        pp = (C.c_void_p * 3)(pin.array.ctypes.data, None, None) if il else (C.c_void_p * 3)(*[pin.array[c].ctypes.data for c in range(3)])
        pin.array[...] = 0
        ctx.call("jxl_vardct_read_output", pp, fr.width)
        t.check(planar(pin.array.copy()), exp, name + ": mapped int16 planes + page-locked read_output")
        t.check(pin.array.copy(), plain, name + ": the same against putGroup + pageable read")
        pin.array[...] = 0
        ctx.call("jxl_vardct_read_output_begin", pp, fr.width)
        ctx.call("jxl_vardct_read_output_wait")
        t.check(planar(pin.array.copy()), exp, name + ": mapped int16 planes + page-locked read_output_begin / _wait")
    finally:
        ctx.synchronize()
        pin.free()


def case_bus():
    from jxlatte_amd import _lib
    t = _Tally()
    lib = _lib.load()
    ctx = _lib.Context(0)
    for name, f in bus_frames():
        _bus_one(t, ctx, lib, name, f)
    ctx.close()
    return t.bad


def _modular_plans():
    """(name, channels, squeeze parameters, adversarial) of the Modular-plan cases"""
    from jxlatte_amd import synth
    from test_modular_gpu import _adversarial
    out = []
    for w, h in ((53, 37), (640, 360), (611, 437)):
        mod = synth.make_modular_frame(w, h, channels=3, seed=w + h)
        out.append(("%dx%dx3" % (w, h), mod["chans"], mod["sp"], False))
    a, r = _adversarial(300, 70)
    out.append(("adversarial h", [a, r], [(1, 1, 0, 1)], True))
    out.append(("adversarial v", [a.T.copy(), r.T.copy()], [(0, 1, 0, 1)], True))
    return out


def run_modular_plans(ctx, orc, check):
    """every plan of _modular_plans on ctx against orc.modular_apply: -> {name: (launches, redos of this plan)}"""
    from jxlatte_amd import host
    seen = {}
    for name, chans, sp, _ in _modular_plans():
        before = ctx.lib.jxl_modular_redo_count(ctx.h)
        out = host.ModularStream(ctx, chans, sp).applyTransforms()
        exp = orc.modular_apply(chans, sp)
        assert len(out) == len(exp), (name, len(out), len(exp))
        for i, (g, e) in enumerate(zip(out, exp)):
            check(g, e, "%s channel %d" % (name, i))
        seen[name] = (ctx.lib.jxl_modular_last_launch_count(ctx.h), ctx.lib.jxl_modular_redo_count(ctx.h) - before)
    return seen


def case_modular():
    """JXL_SQUEEZE_CHAIN_MAX / JXL_SQUEEZE_SHORT_MAX (read once per process): every plan against the oracle; prints launches and
    redos per plan for the parent to compare with the default plan's"""
    from jxlatte_amd import _lib
    from oracle import pyoracle as orc
    t = _Tally()
    ctx = _lib.Context(0)
    for name, (launches, redos) in run_modular_plans(ctx, orc, t.check).items():
        print("PLAN %s | launches %d redos %d" % (name, launches, redos), flush=True)
    ctx.close()
    return t.bad


def case_restore_variants_epf3():
    """JXL_EPF3_SPLIT=0 (read once per process): the three-iteration instantiations of tests/restore_variants.py, single and batch
    launches, against the oracle; the launches each case made are held to the table's, and printed ("SEEN <code>") for the parent
    (tests/test_restore_variants_gpu.py) to add to its inventory"""
    import restore_variants as rv
    t = _Tally()
    ctxs = rv.Contexts()
    seen = set()
    for c in rv.all_cases(child=True):
        try:
            problems = rv.check_case(c, ctxs, t.check, seen)
        except AssertionError as e:
            problems = [str(e)]
        for msg in problems:
            t.bad += 1
            print("FAIL", msg, flush=True)
    for x in sorted(seen):
        print("SEEN", x, flush=True)
    ctxs.close()
    return t.bad


CHILD_CASES = {
    "restore_ph2": case_restore_ph2,
    "restore_ph2_epf3": case_restore_ph2_epf3,
    "restore_lds_pad": case_restore_lds_pad,
    "no_batch_restore": case_no_batch_restore,
    "transfer16": case_transfer16,
    "bus": case_bus,
    "modular": case_modular,
    "restore_variants_epf3": case_restore_variants_epf3,
}

if __name__ == "__main__":
    for path in (ROOT, HERE):
        if path not in sys.path:
            sys.path.insert(0, path)
    failed = CHILD_CASES[sys.argv[1]]()
    print("RESULT", failed, flush=True)
    sys.exit(1 if failed else 0)
