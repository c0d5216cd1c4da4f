"""The patch stage against its independent model (tests/patches_model.py, written from JXLCodestreamDecoder.java:212-254 and
:285-513), on the CPU: the model's own mutation table, today's host path (JXLDecoder._patches over OracleBackend), the type plan
(decoder.patch_type_plan) and the device-free validation (jxl_patch_bins, jxl_canvas_patches_check), all on the shared cases of
tests/patches_model_cases.py. Every comparison of samples is bit equality with the NaNs as one class (conftest.assert_bits_equal):
the inputs hold NaN, +-inf, -0.0 and alphas that make blendBlend divide 0 by 0."""
import types

import numpy as np
import pytest

import patch_ref as R
import patches_model as M
import patches_model_cases as C
from blend_ref import Buf
from conftest import assert_bits_equal
from jxlatte_amd import _lib, abi, decoder, host

F = np.float32
CASES = C.all_cases()


def run_model(case, mut=None):
    """(frame arrays, reference lists of arrays / None, Result, exception or None) of the model on copies of the case's planes"""
    frame = [Buf(a) for a in case.frame]
    ref = [None if r is None else [None if a is None else Buf(a) for a in r] for r in case.reference]
    res, err = None, None
    try:
        res = M.compute_patches(case.info, case.hdr, case.patches, frame, ref, mut=mut)
    except Exception as e:  # noqa: BLE001
        err = e
    return [b.a for b in frame], [None if r is None else [None if b is None else b.a for b in r] for r in ref], res, err


@pytest.fixture(scope="module")
def model():
    return {c.name: run_model(c) for c in CASES}


def _bits(a):
    if a is None:
        return None
    b = a.view(np.uint32) if a.dtype == np.float32 else a
    if a.dtype == np.float32:
        b = np.where(np.isnan(a), np.uint32(0x7FC00000), b)
    return a.dtype.str, a.shape, b.tobytes()


def _outcome(run):
    frame, ref, res, err = run
    return ([_bits(a) for a in frame], [None if r is None else [_bits(a) for a in r] for r in ref],
            None if res is None else sorted(res.created), None if err is None else (type(err).__name__, str(err)))


def fr_of(case):
    hdr = case.hdr
    return types.SimpleNamespace(num_patches=len(case.patches), upsampling=1 if hdr is None else hdr.upsampling,
                                 ec_upsampling=[1] * case.info.num_extra if hdr is None else list(hdr.ec_upsampling))


def assert_same_planes(got_frame, got_ref, exp_frame, exp_ref, what):
    assert len(got_frame) == len(exp_frame)
    for n, (a, b) in enumerate(zip(got_frame, exp_frame)):
        assert_bits_equal(a, b, "%s: frame plane %d" % (what, n), any_nan=True)
    for k in range(4):
        assert (got_ref[k] is None) == (exp_ref[k] is None), (what, k)
        for n, (a, b) in enumerate(zip(got_ref[k] or [], exp_ref[k] or [])):
            assert (a is None) == (b is None), "%s: slot %d plane %d: %s / %s" % (what, k, n, a is None, b is None)
            if a is not None:
                assert_bits_equal(a, b, "%s: slot %d plane %d" % (what, k, n), any_nan=True)


def assert_same_error(got, exp, what):
    """the project's exception against the model's: InvalidBitstreamException with the reference's message"""
    if exp is None:
        assert got is None, (what, got)
        return
    assert isinstance(exp, M.InvalidBitstream), (what, exp)
    assert isinstance(got, (decoder.InvalidBitstreamException, _lib.InvalidBitstreamException)), (what, got)
    assert str(exp) in str(got) if isinstance(got, _lib.JxlError) else str(got) == str(exp), (what, got, exp)


# ---- the cases and the model by themselves ------------------------------------------------------------------------------------
def test_the_model_accepts_every_case_and_the_cases_reach_what_they_must(model):
    kinds, mixed, created, replayed, tags = set(), 0, 0, {5: 0, 7: 0}, set()
    values = set()
    for case in CASES:
        frame, ref, res, err = model[case.name]
        assert err is None or isinstance(err, M.InvalidBitstream), (case, err)  # no TypeClash, no NullPlane, no OutOfPlane: no case skipped
        assert (None if err is None else str(err)) == case.refuse, (case, err)
        tags |= case.tags
        info = case.info
        for p in case.patches:
            if p["ref"] > 3 or case.reference[p["ref"]] is None:
                continue
            slot = case.reference[p["ref"]]
            for j in range(len(p["positions"])):
                for d in range(case.n_chan):
                    c = 0 if d < case.colors else d - case.colors + 1
                    mode, alpha, clamp = (int(v) for v in p["blend"][j][c])
                    if mode == 0:
                        continue
                    kind = "colour" if c == 0 else "alpha" if info.ec_type[c - 1] == 0 else "extra"
                    assoc = bool(info.ec_alpha_associated[alpha]) if info.num_extra else None
                    kinds.add((mode, kind, clamp, assoc))
                    if slot[d] is not None and slot[d].dtype != case.frame[d].dtype:
                        mixed += 1
        if err is None:
            created += len(res.created)
            for m in (5, 7):
                if "below_off%d" % m in case.tags:
                    assert res.replayed, case
                    replayed[m] += 1
            if not any(t.startswith("below_off") for t in case.tags):
                assert not res.replayed, case
        for a in case.frame[case.colors:]:
            if a.dtype == np.float32:
                values |= {("alpha", v) for v in ("nan", "inf", "-inf") if np.any({"nan": np.isnan(a), "inf": a == np.inf, "-inf": a == -np.inf}[v])}
                values |= {("alpha", "0")} if np.any(a == 0) else set()
                values |= {("alpha", "1")} if np.any(a == 1) else set()
                values |= {("alpha", ">1")} if np.any(a[np.isfinite(a)] > 1) else set()
                values |= {("alpha", "<0")} if np.any(a[np.isfinite(a)] < 0) else set()
        for a in case.frame[:case.colors]:
            if a.dtype == np.float32:
                values |= {("sample", "nan")} if np.isnan(a).any() else set()
                values |= {("sample", "inf")} if (a == np.inf).any() else set()
                values |= {("sample", "-inf")} if (a == -np.inf).any() else set()
                values |= {("sample", "-0")} if (a.view(np.uint32) == 0x80000000).any() else set()
    # every mode 1..7 on colour, alpha and non-alpha extra channels, clamp 0 and 1, associated and unassociated alpha
    for mode in range(1, 8):
        for kind in ("colour", "alpha", "extra"):
            here = {(cl, assoc) for m, k, cl, assoc in kinds if m == mode and k == kind}
            assert {cl for cl, _ in here} == {0, 1}, (mode, kind, sorted(here, key=str))
            assert {a for _, a in here} >= {False, True}, (mode, kind, sorted(here, key=str))
    assert {"float", "int", "mixed"} <= tags and mixed > 20           # planes of both types, and frame / reference pairs that differ (:461)
    assert {"absent_planes", "absent_slot", "small_slot", "absent_slot_bad_positions"} <= tags and created > 20
    assert replayed[5] >= 2 and replayed[7] >= 2 and "below_own" in tags
    assert {"colors1", "colors3", "frame37x75", "frame9x33", "1x1", "flush", "tile_edge", "overlap2", "overlap3", "overlap4",
            "order_witness", "zero_over_zero", "mode1", "upsampling", "segments"} <= tags
    assert values >= {("alpha", v) for v in ("0", "1", ">1", "<0", "nan", "inf", "-inf")} | {("sample", v) for v in ("nan", "inf", "-inf", "-0")}, values
    # the witnesses are what they claim to be
    frame, _, _, _ = model["order-witness"]
    assert frame[0][6, 31] == 0.0 and frame[0][5, 29] == F(2.0 ** 24)
    for name in ("zero-alpha-37x75", "zero-alpha-9x33"):
        assert np.isnan(model[name][0][0][0:4, 0:6]).all()  # 0 / 0


def test_every_mutation_changes_a_result(model):
    """the table of deliberately wrong variants: each must differ from the model -- in a sample, a dtype, a created plane or the
    exception -- on at least one shared case; one the cases cannot tell from the model means the cases are too weak"""
    base = {c.name: _outcome(model[c.name]) for c in CASES}
    assert len(M.MUTATIONS) >= 12
    unseen = []
    for mut in M.MUTATIONS:
        if not any(_outcome(run_model(c, mut)) != base[c.name] for c in CASES):
            unseen.append(mut)
    assert not unseen, unseen


# ---- the host path --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def oracle():
    from oracle.pybackend import OracleBackend
    return OracleBackend()


def test_host_path_equals_the_model(model, oracle):
    """JXLDecoder._patches, one backend.blend per application (in pieces for a below mode off its own pixel), over the oracle's
    blend: frame planes and the four reference lists bit for bit, dtypes, the None entries that became planes, and the exception
    -- type, message and, through the planes, the position in stage order at which it came"""
    for case in CASES:
        exp_frame, exp_ref, res, err = model[case.name]
        fb = [a.copy() for a in case.frame]
        ref = [None if r is None else [None if a is None else a.copy() for a in r] for r in case.reference]
        dec = R.shell(case.info, case.patches, ref, oracle)
        got_err = None
        try:
            dec._patches(fr_of(case), fb, case.colors)
        except decoder.InvalidBitstreamException as e:
            got_err = e
        assert_same_error(got_err, err, case.name)
        assert_same_planes(fb, ref, exp_frame, exp_ref, case.name)


def _plan(case):
    return decoder.patch_type_plan(case.info, case.patches, case.frame, case.reference, case.colors, fr_of(case))


def test_type_plan_equals_the_model(model):
    multi = 0
    for case in CASES:
        exp_frame, exp_ref, res, err = model[case.name]
        try:
            plan, got_err = _plan(case), None
        except decoder.InvalidBitstreamException as e:
            plan, got_err = None, e
        assert_same_error(got_err, err, case.name)
        if err is not None:
            continue
        assert plan.frame_types == [a.dtype for a in exp_frame], case
        for k in range(4):
            if k in plan.ref_types:
                assert plan.ref_types[k] == [None if a is None else a.dtype for a in exp_ref[k]], (case, k)
            else:  # no applied patch names the slot: the model left it alone
                for a, b in zip(exp_ref[k] or [], case.reference[k] or []):
                    assert (a is None) == (b is None) and (a is None or a.dtype == b.dtype), (case, k)
        assert plan.created == res.created, case
        assert plan.gather == (not res.replayed), case
        assert len(plan.calls) == res.applications, case
        multi += len(plan.segments) > 1
    assert multi >= 10, multi


def _refused():
    return [c for c in CASES if c.refuse is not None and c.hdr is None]  # (the entries are not told the frame's upsampling: the plan checks it)


def _entry_args(case):
    info = case.info
    pos, blend = R.pos_table(info, case.patches, case.colors)
    is_alpha = [t == 0 for t in info.ec_type[:info.num_extra]]
    assoc = [bool(v) for v in info.ec_alpha_associated[:info.num_extra]]
    return pos, blend, is_alpha, assoc


def _code(a):
    return -1 if a is None else 0 if a.dtype == np.float32 else 1


def test_patch_bins_refuses_what_the_model_refuses(model):
    cases = _refused()
    assert {c.refuse for c in cases} == {"Illegal blend mode", "Patch out of range", "Patch too large", "Patch size out of bounds"}
    for case in cases:
        pos, blend, is_alpha, assoc = _entry_args(case)
        h, w = case.frame[0].shape
        shapes = [None if r is None else tuple(r[0].shape) for r in case.reference]
        rtypes = [[-1] * case.n_chan if r is None else [_code(a) for a in r] for r in case.reference]
        with pytest.raises(_lib.InvalidBitstreamException) as e:
            host.patch_bins(pos, blend, case.colors, is_alpha, assoc, h, w, [_code(a) for a in case.frame], shapes, rtypes)
        assert case.refuse in str(e.value), (case, e.value)
        # the position the entry names is the first one the model did not get past: everything before it was applied
        bad = e.value.position
        before = [dict(p) for p in case.patches]
        n = 0
        for p in before:
            k = max(0, min(len(p["positions"]), bad - n))
            n += len(p["positions"])
            p["positions"], p["blend"] = p["positions"][:k], p["blend"][:k]
        sub = C.Case(case.name + "-prefix", case.colors, case.info, [p for p in before if len(p["positions"])], case.frame, case.reference)
        if case.refuse == "Illegal blend mode":  # (behind the casts and the channels in front of the offending one: types may differ)
            continue
        frame, ref, _, err = run_model(sub)
        assert err is None, (case, err)
        assert_same_planes(frame, ref, model[case.name][0], model[case.name][1], case.name + ": prefix")


def test_canvas_patches_check_refuses_what_the_model_refuses():
    for case in _refused():
        pos, blend, is_alpha, assoc = _entry_args(case)

        def shape_of(planes, like):
            s = abi.CanvasShape()
            s.n, s.h, s.w = case.n_chan, planes[0].shape[0], planes[0].shape[1]
            for n in range(case.n_chan):
                s.types[n] = host._plane_code((planes[n] if planes[n] is not None else like[n]).dtype)
            return s
        fs = shape_of(case.frame, case.frame)
        rs = [None if r is None else shape_of(r, case.frame) for r in case.reference]
        with pytest.raises(_lib.InvalidBitstreamException) as e:
            host.canvas_patches_check(pos, blend, case.colors, is_alpha, assoc, fs, rs)
        assert case.refuse in str(e.value), (case, e.value)
