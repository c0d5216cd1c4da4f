"""The device patch stage against its independent model (tests/patches_model.py), on the GPU: the shared cases of
tests/patches_model_cases.py through jxl_stage_patches (host.computePatches), jxl_planes_patches (ResidentPlanes.patches),
jxl_canvas_patches (the plane-set path, run as tests/test_canvas_patches_gpu.py runs it) and JXLDecoder shells with device_patches
and device_patch_sets. The model is the only yardstick: no oracle and no other entry stands in any assertion.

Samples are compared for bits with the NaNs as one class (conftest.assert_bits_equal(any_nan=True)); pixels outside every applied
position are compared bit for bit, NaN payloads included; dtypes are compared. A list the model answers with an
InvalidBitstreamException is refused with that message before a plane is touched."""
import types

import numpy as np
import pytest

import patch_ref as R
import patches_model as M
import patches_model_cases as C
from blend_ref import Buf
from conftest import assert_bits_equal
from jxlatte_amd import _lib, decoder, host

pytestmark = pytest.mark.gpu
F = np.float32
CASES = C.all_cases()
GPU_CASES = [c for c in CASES if c.colors == 3]
LANDS = "a below mode reads the frame off its own pixel"


def _run_model(case, frame=None, reference=None):
    frame = [Buf(a) for a in (case.frame if frame is None else frame)]
    ref = [None if r is None else [None if a is None else Buf(a) for a in r] for r in (case.reference if reference is None else reference)]
    res, err = None, None
    try:
        res = M.compute_patches(case.info, case.hdr, case.patches, frame, ref)
    except M.InvalidBitstream as e:
        err = e
    return [b.a for b in frame], [None if r is None else [None if b is None else b.a for b in r] for r in ref], res, err


@pytest.fixture(scope="module")
def model():
    """the model's answer to every case, computed once and left alone"""
    out = {c.name: _run_model(c) for c in CASES}
    for frame, ref, _, _ in out.values():
        for a in frame + [b for r in ref if r is not None for b in r if b is not None]:
            a.setflags(write=False)
    return out


@pytest.fixture(scope="module")
def be():
    b = decoder.DeviceBackend()
    yield b
    b.close()


def _copies(case):
    return ([a.copy() for a in case.frame],
            [None if r is None else [None if a is None else a.copy() for a in r] for r in case.reference])


def _fr(case):
    hdr = case.hdr
    return types.SimpleNamespace(num_patches=len(case.patches), upsampling=1 if hdr is None else hdr.upsampling,
                                 ec_upsampling=[1] * case.info.num_extra if hdr is None else list(hdr.ec_upsampling))


def _outside(case):
    """True where no applied position lies"""
    mask = np.ones(case.frame[0].shape, bool)
    for p in case.patches:
        if p["ref"] > 3 or case.reference[p["ref"]] is None:
            continue
        for y0, x0 in p["positions"]:
            mask[max(0, y0):max(0, y0 + p["h"]), max(0, x0):max(0, x0 + p["w"])] = False
    return mask


def _check_frame(case, got, exp, what):
    out = _outside(case)
    for n, (a, b) in enumerate(zip(got, exp)):
        a = np.ascontiguousarray(a)
        assert_bits_equal(a, b, "%s %s: frame plane %d" % (what, case.name, n), any_nan=True)
        assert a[out].tobytes() == b[out].tobytes(), "%s %s: frame plane %d outside the positions" % (what, case.name, n)
        if a.dtype == case.frame[n].dtype:
            assert a[out].tobytes() == case.frame[n][out].tobytes(), "%s %s: frame plane %d outside the positions" % (what, case.name, n)


def _check_lists(case, got, exp, what):
    """reference lists the decoder keeps on the host: the model's, None entries that became planes included"""
    for k in range(4):
        assert (got[k] is None) == (exp[k] is None), (what, case, k)
        for n, (a, b) in enumerate(zip(got[k] or [], exp[k] or [])):
            assert (a is None) == (b is None), "%s %s: slot %d plane %d: %s / %s" % (what, case.name, k, n, a is None, b is None)
            if a is not None:
                assert_bits_equal(a, b, "%s %s: slot %d plane %d" % (what, case.name, k, n), any_nan=True)


def _check_untouched(case, fb, ref, what):
    for n, a in enumerate(fb):
        assert R.same_bits(a, case.frame[n]), (what, case, n)
    for k in range(4):
        for n, a in enumerate(ref[k] or []):
            b = case.reference[k][n]
            assert (a is None) == (b is None) and (a is None or R.same_bits(a, b)), (what, case, k, n)


def _is_refusal(e, msg):
    return isinstance(e, (decoder.InvalidBitstreamException, _lib.InvalidBitstreamException)) and msg in str(e)


# ---- the entries by themselves: planes handed over with the types the reference's casts leave ---------------------------------
def _hoisted(case, model):
    """The stage entries cast nothing: they take the planes with the types blendBuffers' casts would have given them. Where the
    MODEL, run on planes cast beforehand to the types it ends with, gives the very bits it gives on the planes as they are, the
    casts commute with the applications and the entry can be handed those planes. Returns (frame, reference) so cast, or None."""
    exp_frame, exp_ref, res, err = model[case.name]
    if err is not None or res.replayed:
        return None

    def cast(a, like, depth):
        b = Buf(a)
        if like.dtype == np.float32:
            b.cast_to_float(depth)
        return b.a
    info = case.info
    depth = [info.bits_per_sample] * case.colors + list(info.ec_bits[:info.num_extra])
    frame = [cast(a, exp_frame[n], depth[n]) for n, a in enumerate(case.frame)]
    ref = [None if r is None else [None if a is None else cast(a, exp_ref[k][n], depth[n]) for n, a in enumerate(r)]
           for k, r in enumerate(case.reference)]
    again = _run_model(case, frame, ref)
    if again[3] is not None:
        return None
    try:
        for a, b in zip(again[0], exp_frame):
            assert_bits_equal(a, b, any_nan=True)
    except AssertionError:
        return None
    return frame, ref


def _table(case):
    info = case.info
    pos, blend = R.pos_table(info, case.patches, case.colors)
    return pos, blend, [t == 0 for t in info.ec_type[:info.num_extra]], [bool(v) for v in info.ec_alpha_associated[:info.num_extra]]


def test_stage_entry_equals_the_model(ctx, model):
    """jxl_stage_patches, one and three colours"""
    ran = 0
    for case in CASES:
        pos, blend, is_alpha, assoc = _table(case)
        if case.refuse is not None:
            if case.hdr is not None:
                continue  # (the entry is not told the frame's upsampling: patch_type_plan checks it, see the shells below)
            fb, ref = _copies(case)
            with pytest.raises(_lib.InvalidBitstreamException, match=case.refuse):
                host.computePatches(ctx, fb, ref, pos, blend, case.colors, is_alpha, assoc)
            _check_untouched(case, fb, ref, "stage entry")
            continue
        planes = _hoisted(case, model)
        if planes is None:
            continue
        frame, ref = planes
        got = host.computePatches(ctx, [np.ascontiguousarray(a) for a in frame], ref, pos, blend, case.colors, is_alpha, assoc)
        _check_frame(case, got, model[case.name][0], "stage entry")
        ran += 1
    assert ran >= 100, ran


def test_resident_entry_equals_the_model(ctx, model):
    """jxl_planes_patches: float colours in the context's resident planes, the extras beside them"""
    ran = 0
    for case in GPU_CASES:
        planes = None if case.refuse is not None else _hoisted(case, model)
        if planes is None or any(a.dtype != np.float32 for a in planes[0][:3]):
            continue
        frame, ref = planes
        pos, blend, is_alpha, assoc = _table(case)
        rp = host.ResidentPlanes.upload(ctx, np.stack(frame[:3]))
        extras = [np.ascontiguousarray(a) for a in frame[3:]]
        rp.patches(extras, ref, pos, blend, is_alpha, assoc)
        _check_frame(case, list(rp.download()) + extras, model[case.name][0], "resident entry")
        ran += 1
    assert ran >= 50, ran


# ---- the decoder's three routes ---------------------------------------------------------------------------------------------
def _shell_device(case, backend):
    """the patch stage of _chained_tail with device_patches: _patches_device, and the blend calls where it declines"""
    fb, ref = _copies(case)
    dec = R.shell(case.info, case.patches, ref, backend)
    planes = decoder.FramePlanes(backend, case.info, fb, 3)
    took = dec._patches_device(_fr(case), planes)
    if not took:
        dec._patches(_fr(case), planes.to_host(), 3)
    return [np.ascontiguousarray(a) for a in planes.to_host()], ref, took, dec.stats[-1].get("patches", {})


@pytest.mark.parametrize("which", ["stage entry", "resident planes"])
def test_device_patches_shell_equals_the_model(ctx, be, model, which):
    """JXLDecoder(device_patches=True)'s stage, with the casts and segments of patch_type_plan: over a backend that has only the
    stage entry, and over DeviceBackend, which keeps float colours resident"""
    backend = types.SimpleNamespace(patches=lambda *a: host.computePatches(ctx, *a), blend=be.blend) if which == "stage entry" else be
    multi = declined = 0
    for case in GPU_CASES:
        exp_frame, exp_ref, res, err = model[case.name]
        if err is not None:
            fb, ref = _copies(case)
            dec = R.shell(case.info, case.patches, ref, backend)
            with pytest.raises((decoder.InvalidBitstreamException, _lib.InvalidBitstreamException)) as e:
                dec._patches_device(_fr(case), decoder.FramePlanes(backend, case.info, fb, 3))
            assert _is_refusal(e.value, str(err)), (case, e.value)
            _check_untouched(case, fb, ref, which)
            continue
        got, ref, took, st = _shell_device(case, backend)
        assert took == (not res.replayed), (case, st)
        _check_frame(case, got, exp_frame, which)
        _check_lists(case, ref, exp_ref, which)
        multi += st.get("segments", 0) > 1
        declined += not took
    assert multi >= 10 and declined >= 6, (multi, declined)


def _on_sets(be, case):
    """the patch stage on plane sets, as tests/test_canvas_patches_gpu.py runs it: the frame's planes go up with
    FramePlanes.adopt_set, every slot is a DeviceCanvas (an absent plane a zero plane of the type the model creates it with, or of
    the frame plane's). Returns (why, frame planes, per slot the planes downloaded or None, stats row, the frame's arrays)"""
    ctx = be.ctx
    fb, lists = _copies(case)
    sets = []
    for r in lists:
        if r is None:
            sets.append(None)
            continue
        sets.append(host.DeviceCanvas.fromArrays(ctx, [np.zeros(r[0].shape, fb[n].dtype) if a is None else a for n, a in enumerate(r)]))
    dec = R.shell(case.info, case.patches, list(sets), be)
    dec._dead_sets = []
    planes = decoder.FramePlanes(be, case.info, fb, 3)
    try:
        why = dec._patches_sets(_fr(case), planes)
        out = fb if planes.set is None else [planes.set.download(c) for c in range(len(planes.set))]
        refs = [None if s is None else [s.download(c) for c in range(len(s))] for s in sets]
        return why, out, refs, dec.stats[-1].get("patches", {}), fb
    finally:
        dec._release_dead()
        for s in sets:
            if s is not None:
                s.release()
        if planes.set is not None:
            planes.set.release()


def test_plane_set_path_equals_the_model(be, model):
    """jxl_canvas_patches + jxl_canvas_cast_planes under JXLDecoder(device_patch_sets=True)'s stage: the frame set and the slots'
    sets afterwards are the model's planes, dtypes included; a slot's plane that was absent reads as zeros and stays zeros"""
    multi = landed = 0
    for case in GPU_CASES:
        exp_frame, exp_ref, res, err = model[case.name]
        if err is not None:
            with pytest.raises((decoder.InvalidBitstreamException, _lib.InvalidBitstreamException)) as e:
                _on_sets(be, case)
            assert _is_refusal(e.value, str(err)), (case, e.value)
            continue
        why, got, refs, st, fb = _on_sets(be, case)
        if res.replayed:  # nothing touched: the caller lands the canvas and runs the blend calls
            assert why == LANDS, (case, why)
            _check_untouched(case, got, [None] * 4, "plane sets")
            for k, r in enumerate(refs):
                for n, a in enumerate(r or []):
                    b = case.reference[k][n]
                    assert R.same_bits(a, b) if b is not None else not a.view(np.uint32).any(), (case, k, n)
            landed += 1
            continue
        assert why is None, (case, why)
        _check_frame(case, got, exp_frame, "plane sets")
        for k, r in enumerate(refs):
            assert (r is None) == (exp_ref[k] is None), (case, k)
            for n, a in enumerate(r or []):
                b = exp_ref[k][n]
                if case.reference[k][n] is None:  # absent in the slot: zeros, whether or not the reference made the plane
                    assert not a.view(np.uint32).any(), (case, k, n)
                    assert b is None or not b.view(np.uint32).any(), (case, k, n)
                else:
                    assert_bits_equal(a, b, "plane sets %s: slot %d plane %d" % (case.name, k, n), any_nan=True)
        multi += st.get("segments", 0) > 1
    assert multi >= 10 and landed >= 6, (multi, landed)
