"""Every documented run-time switch that selects other device code or another launch plan, forced and held to the bar of the default
path: the oracle's bits (the f64 transfer forms: the bars tests/test_stages_gpu.py states for them). The list of switches and the
bodies of the child processes are in tests/switch_cases.py; tests/test_switch_inventory_cpu.py keeps the list complete.

How a switch is set follows how the library reads it: once per process -> a fresh child process (one at a time, each under its own
time limit); per context -> monkeypatch and a fresh context; per call or per plan -> monkeypatch on the session context.
A child that dies of a signal, aborts, or runs into its time limit fails its test, and every later child test of the module is
skipped with that failure as the reason: what faulted is not started again.

The switches of the existing suites are not repeated here; PINNED_ELSEWHERE names their tests."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import switch_cases as sc
from conftest import assert_bits_equal
from jxlatte_amd import _lib, abi, host, synth
from test_modular_gpu import _adversarial, _vh_inputs
from test_stages_gpu import ulp_diff

pytestmark = pytest.mark.gpu

PINNED_ELSEWHERE = {name: where for name, where in sc.RESULT_PATH.items() if not where.startswith("test_switches_gpu.py::")}
# JXL_EPF3_SPLIT, JXL_WG3_GRID, JXL_WG3_GRID_BIG, JXL_SHARED_PLANES, JXL_HSQUEEZE_WALK_MAX, JXL_SQUEEZE_SPECULATE, JXL_SQUEEZE_NO_VH,
# JXL_VH_SEG, JXL_VH_CW

_first_child_failure = None  # the first child that faulted or hung: no child is started after it


def run_child(case, env, timeout):
    """switch_cases.py <case> in a fresh process with `env` added; -> its stdout. Fails the test unless it exits 0 with RESULT 0."""
    global _first_child_failure
    if _first_child_failure:
        pytest.skip("no child process after a fault: " + _first_child_failure)
    e = dict(os.environ)
    for k in sc.RESULT_PATH:  # a child sees the switches of its case only
        e.pop(k, None)
    e.update(env)
    tag = "%s %s" % (case, " ".join("%s=%s" % kv for kv in sorted(env.items())))
    try:
        r = subprocess.run([sys.executable, os.path.join(sc.HERE, "switch_cases.py"), case], env=e, capture_output=True, text=True, timeout=timeout)
    except subprocess.TimeoutExpired as ex:
        _first_child_failure = "%s ran into its time limit of %d s" % (tag, timeout)
        pytest.fail(_first_child_failure + "\n" + str(ex.stdout)[-2000:])
    if r.returncode < 0 or r.returncode in (134, 139, 124, 137):
        _first_child_failure = "%s ended with status %d" % (tag, r.returncode)
        pytest.fail(_first_child_failure + "\n" + r.stdout[-2000:] + r.stderr[-2000:])
    assert r.returncode == 0 and "RESULT 0" in r.stdout.split("\n"), tag + "\n" + "\n".join(
        ln for ln in r.stdout.split("\n") if not ln.startswith("ok  "))[-3000:] + r.stderr[-2000:]
    return r.stdout


@pytest.fixture
def no_switches(monkeypatch):
    """the per-call and per-context switches of this module unset, whatever the caller's environment holds"""
    for k in sc.RESULT_PATH:
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


# ---- restoration kernel ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,env", [("restore_ph2", {}), ("restore_ph2_epf3", {}), ("restore_ph2_epf3", {"JXL_EPF3_SPLIT": "0"})],
                         ids=["epf0-3", "epf3-split", "epf3-one-launch"])
def test_restore_4x2_patches(case, env):
    """JXL_RESTORE_PH=2: the k_restore_fused<GAB, ITERS, SK_PLAIN, 2> instantiations (256 threads, 4x2 register patches) on every
    (Gaborish, EPF iterations) combination, stage sets 7 and 15 with float planes out, frame edges on both sides of every tile
    geometry (switch_cases.RESTORE_SIZES), and a three-frame batch (the batch kernel has 4x1 patches only). Three iterations run
    as the default pair of launches -- the second is the two-iteration kernel on 4x2 patches -- and as one launch (JXL_EPF3_SPLIT=0).
    The library has no counter that tells the patch forms apart: the test pins that the results are the oracle's with the variable
    set. That the variable selects the 4x2 kernels was seen once in a kernel trace of these children (rocprofv3 --kernel-trace --stats):
    k_restore_fused<true|false, 0|1|2, 0, 2> for zero to two iterations; for three, k_restore_fused<true|false, 4, 0, 1> (the 13-tap
    half has 4x1 patches only) followed by k_restore_fused<false, 2, 0, 2>, and with JXL_EPF3_SPLIT=0 k_restore_fused<true|false, 3, 0, 2>;
    the batches ran k_restore_fused_batch<true, 2|3, 0>. No <.., 0, 1> instantiation of zero to three iterations appeared."""
    run_child(case, dict(env, JXL_RESTORE_PH="2"), 240)


def test_restore_lds_pad():
    """JXL_RESTORE_LDS_PAD: 16 KiB of extra dynamic LDS on every fused restoration launch (the attribute and the launch both carry
    it; switch_cases.LDS_PAD_BYTES says why it fits). One and two iterations at (136, 72) and (520, 264), plus the batch. No counter
    shows the padding: the test pins that the results stay the oracle's with the variable set. (A kernel trace does not show it
    either: the same k_restore_fused<true|false, 1|2, 0, 1> and k_restore_fused_batch<true, 2, 0> with and without the variable, and
    its LDS column reads 0 for dynamic LDS both times. That the bytes reach the launch is read from launch_tph.)"""
    run_child("restore_lds_pad", {"JXL_RESTORE_LDS_PAD": str(sc.LDS_PAD_BYTES)}, 180)


# ---- side streams ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def two_launch_frames(orc):
    """frames with a second IDCT launch: 64x32 / 32x64 blocks beside 8x8 ones (the 512-thread class on the side stream), and 4:2:0
    (per-channel launches dealt over the side streams); with the oracle's planes"""
    mixed = synth.make_vardct_frame(264, 136, seed=51, mix="DCT8=0.4+DCT64_32=0.3+DCT32_64=0.3")
    sub = synth.make_subsampled(synth.make_vardct_frame(272, 144, seed=52, mix="dct8", xyb=0), (1, 0, 1), (1, 0, 1))
    return [("64x32 mix", mixed, 15, orc.vardct_frame(mixed, stages=15)), ("4:2:0", sub, 7, orc.vardct_frame(sub, stages=7))]


@pytest.mark.parametrize("n_aux", [0, 2, sc.AUX_MAX])
def test_aux_streams(orc, two_launch_frames, n_aux, no_switches):
    """JXL_AUX_STREAMS (read when a context is created): no side stream, two, and all jxl_ctx::kAux of them. Twice per frame: the
    second run finds the streams and events of the first in use. No counter shows where a launch went: the test pins the results.
    (Seen once in a kernel trace of these two frames: with 0 every launch on one stream; with 2, k_idct_wg3<true> -- the 512-thread
    class -- on a second stream and the three k_idct_multi<0> launches of the 4:2:0 frame on three streams.)"""
    no_switches.setenv("JXL_AUX_STREAMS", str(n_aux))
    c = _lib.Context(0)
    try:
        for name, frame, st, exp in two_launch_frames:
            fr = host.Frame.from_synth(c, frame, stages=st)
            for run in range(2):
                assert_bits_equal(fr.decodeFrame(), exp, "%s with %d side streams, run %d" % (name, n_aux, run))
            assert fr.lastLaunchCount() >= 3  # two IDCT launches at least, and the restoration launch
    finally:
        c.close()


@pytest.mark.parametrize("horizontal", [True, False])
def test_aux_streams_none_turns_side_stream_checks_into_in_order_repair(orc, horizontal, no_switches):
    """JXL_AUX_STREAMS=0 with JXL_SQUEEZE_SPECULATE=1: there is no side stream for the checks, so the plan runs as mode 0 -- rows that
    never forget their start are repaired by the step's own verification launch: the serial walk's result, and no second run"""
    no_switches.setenv("JXL_AUX_STREAMS", "0")
    no_switches.setenv("JXL_SQUEEZE_SPECULATE", "1")
    a, r = _adversarial(300, 70)
    exp = orc.inv_hsqueeze(a, r)
    if not horizontal:
        a, r, exp = a.T.copy(), r.T.copy(), exp.T.copy()
    c = _lib.Context(0)
    try:
        before = c.lib.jxl_modular_redo_count(c.h)
        out = host.ModularStream(c, [a, r], [(1 if horizontal else 0, 1, 0, 1)]).applyTransforms()
        assert_bits_equal(out[0], exp, "adversarial rows without side streams")
        assert c.lib.jxl_modular_redo_count(c.h) == before
    finally:
        c.close()


# ---- batch ----------------------------------------------------------------------------------------------------------------------
def _batch(frames, exps, what, batch=True):
    """the frames on a context each, as one batch or singly, each against the oracle: -> summed launch count"""
    ctxs = [_lib.Context(0) for _ in frames]
    try:
        frs = [host.Frame.from_synth(c, f, stages=15) for c, f in zip(ctxs, frames)]
        if batch:
            host.Frame.runBatch(frs)
        else:
            for fr in frs:
                fr.run()
        for i, (fr, e) in enumerate(zip(frs, exps)):
            assert_bits_equal(fr.readOutput(), e, "%s, frame %d" % (what, i))
        return sum(fr.lastLaunchCount() for fr in frs)
    finally:
        for c in ctxs:
            c.close()


@pytest.fixture(scope="module")
def batches(orc):
    """both batches of switch_cases.batch_frames with the oracle's planes, and the launches of the one-variant batch's frames run singly"""
    out = {}
    for kind in ("mixed", "one"):
        frames = sc.batch_frames(kind)
        out[kind] = (frames, [orc.vardct_frame(f, stages=15) for f in frames])
    out["single"] = _batch(out["one"][0], out["one"][1], "frames run singly", batch=False)
    return out


def test_no_batch(batches, no_switches):
    """JXL_NO_BATCH=1 (read per call): jxl_vardct_run_batch runs its frames one by one -- as many launches as the frames run singly,
    where the batch shares its IDCT and restoration launches and so has fewer. Four frames of differing restoration variants and
    four of one variant: the oracle's planes either way."""
    default = {k: _batch(batches[k][0], batches[k][1], "%s batch" % k) for k in ("mixed", "one")}
    assert default["one"] < batches["single"], (default, batches["single"])
    no_switches.setenv("JXL_NO_BATCH", "1")
    for k in ("mixed", "one"):
        n = _batch(batches[k][0], batches[k][1], "%s batch, JXL_NO_BATCH=1" % k)
        if k == "one":
            assert n == batches["single"], (n, batches["single"])
        else:
            assert n > default[k], (n, default)


def test_no_batch_restore(batches, no_switches):
    """JXL_NO_BATCH_RESTORE=1 (read once per process: a child): the batch shares its IDCT launches only, every frame launches its own
    restoration kernel. Launches of the one-variant batch: more than the default batch (one restoration launch for all four), fewer
    than the frames run one by one (an IDCT launch each)."""
    default = _batch(batches["one"][0], batches["one"][1], "one-variant batch")
    out = run_child("no_batch_restore", {"JXL_NO_BATCH_RESTORE": "1"}, 120)
    counts = {m.group(1): int(m.group(2)) for m in re.finditer(r"^COUNT (\w+) (\d+)$", out, re.M)}
    assert default < counts["one"] < batches["single"], (default, counts, batches["single"])


# ---- transfer functions ---------------------------------------------------------------------------------------------------------
def _code_diff(got, exp):
    d = np.abs(sc.planar(got).astype(np.int64) - exp)
    return int(d.max()), float((d != 0).mean())


def _exact_forms_equal_the_oracle(ctx, orc, x):
    """with no switch set the quantised outputs are the oracle's integers, for the inputs the switched forms are measured on"""
    for tf, maxv in ((abi.TRANSFER_PQ, 65535), (abi.TRANSFER_PQ, 255), (abi.TRANSFER_SRGB, 65535), (abi.TRANSFER_SRGB, 255)):
        assert_bits_equal(host.transfer(ctx, x, tf, maxv), orc.transfer(x, tf, maxv), "default form, transfer %d to %d" % (tf, maxv))
    for f, tf, fmt in sc.sink_frames():
        assert_bits_equal(sc.planar(host.Frame.from_synth(ctx, f).decodeFrame()), orc.vardct_frame(f), "default sink, transfer %d %s" % (tf, fmt))


def test_f64_transfer_forms_per_context(ctx, orc, no_switches):
    """JXL_PQ_F64 / JXL_SRGB8_F64 (read when a context is created): the f64 pow forms instead of the PQ segment table and the sRGB 8-bit
    threshold table. Bars: PQ -- that of test_transfer_pq_exact_form (<= 1 ulp, under 1e-4 of the floats and 1e-5 of the code values
    differ; the table form differs in a few per cent of the floats, so meeting it shows the switch took effect); sRGB to 8 bits --
    within one code value, under 1e-3 differing (test_transfer_within_one_ulp). Through jxl_stage_transfer and through the frame
    sink (stage set 31, the four integer formats); and the default forms equal the oracle on the same inputs."""
    x = sc.transfer_inputs()
    _exact_forms_equal_the_oracle(ctx, orc, x)
    table = ulp_diff(host.transfer(ctx, x, abi.TRANSFER_PQ), orc.transfer(x, abi.TRANSFER_PQ))
    assert (table != 0).mean() > 1e-3  # (the table form on these inputs: what the f64 form must not look like)
    frames = sc.sink_frames()

    no_switches.setenv("JXL_PQ_F64", "1")
    c = _lib.Context(0)
    try:
        d = ulp_diff(host.transfer(c, x, abi.TRANSFER_PQ), orc.transfer(x, abi.TRANSFER_PQ))
        print("JXL_PQ_F64 float: max %d ulp, share %.2e" % (d.max(), (d != 0).mean()))
        assert d.max() <= 1 and (d != 0).mean() < 1e-4, (d.max(), (d != 0).mean())
        for maxv in (65535, 255):
            mx, share = _code_diff(host.transfer(c, x, abi.TRANSFER_PQ, maxv), orc.transfer(x, abi.TRANSFER_PQ, maxv))
            print("JXL_PQ_F64 to %d: max %d, share %.2e" % (maxv, mx, share))
            assert mx <= 1 and share < 1e-5, (maxv, mx, share)
        for f, tf, fmt in frames:
            if tf == abi.TRANSFER_PQ:
                mx, share = _code_diff(host.Frame.from_synth(c, f).decodeFrame(), orc.vardct_frame(f))
                print("JXL_PQ_F64 sink %s %dx%d: max %d, share %.2e" % (fmt, f["width"], f["height"], mx, share))
                assert mx <= 1 and share < 1e-5, (fmt, mx, share)
    finally:
        c.close()

    no_switches.delenv("JXL_PQ_F64")
    no_switches.setenv("JXL_SRGB8_F64", "1")
    c = _lib.Context(0)
    try:
        mx, share = _code_diff(host.transfer(c, x, abi.TRANSFER_SRGB, 255), orc.transfer(x, abi.TRANSFER_SRGB, 255))
        print("JXL_SRGB8_F64 to 255: max %d, share %.2e" % (mx, share))
        assert mx <= 1 and share < 1e-3, (mx, share)
        for f, tf, fmt in frames:
            if tf == abi.TRANSFER_SRGB and fmt in ("U8", "RGB8"):
                mx, share = _code_diff(host.Frame.from_synth(c, f).decodeFrame(), orc.vardct_frame(f))
                print("JXL_SRGB8_F64 sink %s %dx%d: max %d, share %.2e" % (fmt, f["width"], f["height"], mx, share))
                assert mx <= 1 and share < 1e-3, (fmt, mx, share)
    finally:
        c.close()


def test_f64_transfer_forms_16_bit(ctx, orc, no_switches):
    """JXL_PQ16_F64 / JXL_SRGB16_F64 (read once per process: one child with both, they touch different transfer functions): 16-bit
    code values from the quantised float instead of the threshold tables -- within one code value of the oracle, under 1e-3 of them
    differing (test_transfer_within_one_ulp's limit for quantised output), through jxl_stage_transfer and the frame sink (U16,
    RGB16). In this process, with the switches unset, the same inputs give the oracle's integers exactly."""
    _exact_forms_equal_the_oracle(ctx, orc, sc.transfer_inputs())
    out = run_child("transfer16", {"JXL_PQ16_F64": "1", "JXL_SRGB16_F64": "1"}, 120)
    rows = re.findall(r"^DIFF (.+) max (\d+) share (\S+)$", out, re.M)
    assert len(rows) == 2 + 8, out[-2000:]
    print("\n".join("%s: max %s, share %s" % r for r in rows))
    for what, mx, share in rows:
        assert int(mx) <= 1 and float(share) < 1e-3, (what, mx, share)


# ---- bus paths ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", [{"JXL_COMMIT_ZEROCOPY": "0", "JXL_TABLE_ZEROCOPY": "0", "JXL_OUTPUT_ZEROCOPY": "0"},
                                 {"JXL_WIDEN_GRID": "1", "JXL_OUTPUT_GRID": "1"}, {"JXL_WIDEN_GRID": "7", "JXL_OUTPUT_GRID": "7"}],
                         ids=["staged", "grid1", "grid7"])
def test_bus_paths(env):
    """the streaming boundary the other way: the staged forms (SDMA copy + k_widen2d, hipMemcpyAsync for tables and results) instead of
    kernels over the page-locked aliases; and the transfer kernels on one workgroup and on seven -- no divisor of the tile counts, so
    the grid-stride loops end on a partial round. Frames through the mapped int16 planes (jxl_vardct_map_coeffs_i16 / commit) into a
    page-locked destination, both read_output forms: the oracle's bits, and those of putGroup + a pageable read (switch_cases.bus_frames:
    (264, 136), (1000, 520), float / interleaved 8-bit / planar 16-bit results, one 4:2:0 frame). No counter shows which path a copy
    took: the test pins the results. (Seen once in a kernel trace of the first child: k_widen2d where the default run has
    k_widen2d_host8, no k_copy16 at all where the default run has it for tables and results, and twice the copyBuffer calls.)"""
    run_child("bus", env, 180)


# ---- Modular plan ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def default_plans(ctx, orc):
    """launches and redos of every plan of switch_cases._modular_plans with no switch set"""
    saved = {k: os.environ.pop(k) for k in list(os.environ) if k in sc.RESULT_PATH}
    try:
        return sc.run_modular_plans(ctx, orc, assert_bits_equal)
    finally:
        os.environ.update(saved)


FRAMES = ("53x37x3", "640x360x3", "611x437x3")
ADVERSARIAL = ("adversarial h", "adversarial v")


def test_default_plans_are_what_the_switch_tests_assume(default_plans):
    assert all(default_plans[k][1] == 0 for k in FRAMES) and all(default_plans[k][1] == 1 for k in ADVERSARIAL), default_plans


def test_squeeze_no_chain(ctx, orc, default_plans, no_switches):
    """JXL_SQUEEZE_NO_CHAIN=1 (per plan): the small leading steps as launches of their own instead of one k_squeeze_chain launch"""
    no_switches.setenv("JXL_SQUEEZE_NO_CHAIN", "1")
    seen = sc.run_modular_plans(ctx, orc, assert_bits_equal)
    for k in FRAMES:
        assert seen[k][0] > default_plans[k][0], (k, seen[k], default_plans[k])
    assert all(seen[k][1] == default_plans[k][1] for k in seen), (seen, default_plans)


def _child_plans(env):
    out = run_child("modular", env, 120)
    return {m.group(1): (int(m.group(2)), int(m.group(3))) for m in re.finditer(r"^PLAN (.+) \| launches (\d+) redos (\d+)$", out, re.M)}


@pytest.mark.parametrize("chain_max", [1, 4096])
def test_squeeze_chain_max(default_plans, chain_max):
    """JXL_SQUEEZE_CHAIN_MAX (once per process): 1 -- only steps of one pair may join the chain, so it ends early and the plan has more
    launches (at least as many; more where the default chain held longer steps); 4096 -- every leading step with <= 256 lanes joins:
    fewer launches or as many"""
    seen = _child_plans({"JXL_SQUEEZE_CHAIN_MAX": str(chain_max)})
    assert set(seen) == set(default_plans)
    for k in FRAMES:
        if chain_max == 1:
            assert seen[k][0] >= default_plans[k][0], (k, seen[k], default_plans[k])
        else:
            assert seen[k][0] <= default_plans[k][0], (k, seen[k], default_plans[k])
    moved = [k for k in FRAMES if seen[k][0] != default_plans[k][0]]
    assert moved, (seen, default_plans)  # the limit did something
    assert all(seen[k][1] == default_plans[k][1] for k in seen), (seen, default_plans)


@pytest.mark.parametrize("short_max", [0, 1 << 40])
def test_squeeze_short_max(default_plans, short_max):
    """JXL_SQUEEZE_SHORT_MAX (once per process): 0 -- every segmented step on the default geometry (64-pair segments, 16 warm-up pairs);
    huge -- every one on the short geometry (32 / 8). The adversarial rows mismatch at every boundary of either: redone exactly once"""
    seen = _child_plans({"JXL_SQUEEZE_SHORT_MAX": str(short_max)})
    assert set(seen) == set(default_plans)
    assert all(seen[k][1] == 1 for k in ADVERSARIAL) and all(seen[k][1] == 0 for k in FRAMES), seen


def test_squeeze_no_tail(ctx, orc, default_plans, no_switches):
    """JXL_SQUEEZE_NO_TAIL=1 (per plan): no compact tail arrays, so a segmented step cannot hand its check to the next walk launch: it is
    checked and repaired in place by its own verification launch (run_modular_plan, kind 4). The adversarial rows come out as the
    serial walk's -- redone by that launch, with no second run of the plan, where the default plan reports and runs again -- and
    ordinary rows are left alone"""
    no_switches.setenv("JXL_SQUEEZE_NO_TAIL", "1")
    seen = sc.run_modular_plans(ctx, orc, assert_bits_equal)
    assert all(seen[k][1] == 0 for k in seen), seen
    assert all(default_plans[k][1] == 1 for k in ADVERSARIAL)  # (the same rows do trip the default plan)


def test_squeeze_serial_small(ctx, orc, default_plans, no_switches):
    """JXL_SQUEEZE_SERIAL=1 (per plan) at small sizes: one serial walk per row / column, no segment states -- nothing to mismatch"""
    no_switches.setenv("JXL_SQUEEZE_SERIAL", "1")
    seen = sc.run_modular_plans(ctx, orc, assert_bits_equal)
    assert all(seen[k][1] == 0 for k in seen), seen


@pytest.mark.parametrize("name,value", [("JXL_VH_TILES", "1"), ("JXL_VH_TILES", "1000000"), ("JXL_VH_SMALL", "0"), ("JXL_VH_SMALL", "1000000000"),
                                        ("JXL_VH_CW32_MINSEG", "16"), ("JXL_VH_CW32_MINSEG", "1000000")])
def test_vh_geometry(ctx, orc, name, value, no_switches):
    """segment length and chunk width of the fused V + H kernel (k_inv_vh / k_inv_vh32; make_vh in host.hip, read per plan): the tile
    count the segment length aims at (1: 256-pair segments, 10^6: 32), the tile count under which 32-pair segments become 16-pair
    ones (0: never, 10^9: always), the segment length from which the wide chunk form runs (16: always, 10^6: never) -- on the
    default plans of two images and on pair plans with odd sizes, which must still be the fused launch"""
    no_switches.setenv(name, value)
    for w, h in ((640, 360), (611, 437)):
        mod = synth.make_modular_frame(w, h, channels=3, seed=w + h)
        before = ctx.lib.jxl_modular_redo_count(ctx.h)
        out = host.ModularStream(ctx, mod["chans"], mod["sp"]).applyTransforms()
        for i, (g, e) in enumerate(zip(out, orc.modular_apply(mod["chans"], mod["sp"]))):
            assert_bits_equal(g, e, "%dx%d channel %d, %s=%s" % (w, h, i, name, value))
        assert ctx.lib.jxl_modular_redo_count(ctx.h) == before
    for htot, wtot in ((130, 257), (321, 514)):
        chans, sp = _vh_inputs(np.random.default_rng(htot * 131 + wtot), htot, wtot)
        out = host.ModularStream(ctx, chans, sp).applyTransforms()
        assert_bits_equal(out[0], orc.modular_apply(chans, sp)[0], "pair %dx%d, %s=%s" % (htot, wtot, name, value))
        assert ctx.lib.jxl_modular_last_launch_count(ctx.h) <= 2  # the pair + (at most) one check launch: the fused kernel ran
